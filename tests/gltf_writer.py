"""Test-side glTF 2.0 writer: builds .gltf + .bin, data-URI .gltf and .glb files from numpy arrays with chosen
component types, strides and offsets, so that the reader's container and accessor rules (rsd/gltf.py) are tested on
inputs whose content is known.  Also a minimal PNG encoder for alpha textures.  Test infrastructure only."""
import base64
import json
import struct
import zlib
from pathlib import Path

import numpy as np

BYTE, UBYTE, SHORT, USHORT, UINT, FLOAT = 5120, 5121, 5122, 5123, 5125, 5126
DTYPE = {BYTE: "<i1", UBYTE: "<u1", SHORT: "<i2", USHORT: "<u2", UINT: "<u4", FLOAT: "<f4"}
TYPE_OF_WIDTH = {1: "SCALAR", 2: "VEC2", 3: "VEC3", 4: "VEC4", 16: "MAT4"}


def png(pixels) -> bytes:
    """uint8 [h, w, c] (c = 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA) as an 8-bit PNG, filter 0 rows."""
    px = np.asarray(pixels, np.uint8)
    h, w, c = px.shape
    raw = b"".join(b"\x00" + px[y].tobytes() for y in range(h))

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))

    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


class Writer:
    """A glTF document under construction: `doc` is the JSON (edit it freely), `blob` the one binary buffer."""

    def __init__(self):
        self.doc = {"asset": {"version": "2.0"}}
        self.blob = bytearray()

    def add(self, key, obj) -> int:
        self.doc.setdefault(key, []).append(obj)
        return len(self.doc[key]) - 1

    def view(self, data: bytes, stride=None, lead=0) -> int:
        """A bufferView of `data`, 4-byte aligned, after `lead` bytes of filler (a non-zero byteOffset)."""
        self.blob += b"\xAB" * (lead + (-(len(self.blob) + lead)) % 4)
        v = {"buffer": 0, "byteOffset": len(self.blob), "byteLength": len(data)}
        if stride:
            v["byteStride"] = stride
        self.blob += data
        return self.add("bufferViews", v)

    def accessor(self, array, component=FLOAT, normalized=False, lead=0, skip=0, atype=None) -> int:
        """`array` [count, width] (or [count]) stored tightly as `component`; a normalised integer type stores
        round(x * max).  lead: filler bytes before the view; skip: the accessor's own byteOffset (filler inside the
        view, a multiple of the component size)."""
        a = np.asarray(array)
        a = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(-1, 1)
        dt = np.dtype(DTYPE[component])
        if normalized and component != FLOAT:
            a = np.round(a.astype(np.float64) * np.iinfo(dt).max)
        data = b"\xCD" * skip + np.ascontiguousarray(a.astype(dt)).tobytes()
        acc = {"bufferView": self.view(data, lead=lead), "componentType": component, "count": int(a.shape[0]),
               "type": atype or TYPE_OF_WIDTH[a.shape[1]]}
        if skip:
            acc["byteOffset"] = skip
        if normalized:
            acc["normalized"] = True
        if atype is None and a.shape[1] == 3 and component == FLOAT:
            acc["min"], acc["max"] = a.min(0).astype(float).tolist(), a.max(0).astype(float).tolist()
        return self.add("accessors", acc)

    def interleaved(self, arrays, stride, lead=0):
        """float32 arrays of one count interleaved in one view of `stride` bytes per element (>= their widths, the
        rest filler); returns one accessor per array."""
        arrays = [np.asarray(a, "<f4").reshape(len(a), -1) for a in arrays]
        n = arrays[0].shape[0]
        rows = np.full((n, stride), 0xEF, np.uint8)
        offs, o = [], 0
        for a in arrays:
            rows[:, o:o + 4 * a.shape[1]] = a.view(np.uint8).reshape(n, -1)
            offs.append(o)
            o += 4 * a.shape[1]
        assert o <= stride
        view = self.view(rows.tobytes(), stride=stride, lead=lead)
        out = []
        for a, o in zip(arrays, offs):
            acc = {"bufferView": view, "componentType": FLOAT, "count": n, "type": TYPE_OF_WIDTH[a.shape[1]]}
            if o:
                acc["byteOffset"] = o
            out.append(self.add("accessors", acc))
        return out

    def image(self, data: bytes, mime=None, embed=True) -> int:
        """An image from a bufferView (embed) or a data URI."""
        if embed:
            img = {"bufferView": self.view(data), "mimeType": mime or "image/png"}
        else:
            img = {"uri": f"data:{mime or 'image/png'};base64," + base64.b64encode(data).decode()}
        return self.add("images", img)

    def save(self, path, container="gltf") -> Path:
        """container: "gltf" (JSON + a .bin file beside it), "datauri" (JSON with the buffer inline), "glb"."""
        path = Path(path)
        doc = json.loads(json.dumps(self.doc))
        blob = bytes(self.blob) + b"\x00" * (-len(self.blob) % 4)
        if blob:
            doc["buffers"] = [{"byteLength": len(blob)}]
        if container == "glb":
            js = json.dumps(doc).encode()
            js += b" " * (-len(js) % 4)
            body = struct.pack("<II", len(js), 0x4E4F534A) + js
            if blob:
                body += struct.pack("<II", len(blob), 0x004E4942) + blob
            path.write_bytes(struct.pack("<III", 0x46546C67, 2, 12 + len(body)) + body)
            return path
        if blob and container == "gltf":
            bin_path = path.with_suffix(".bin")
            bin_path.write_bytes(blob)
            doc["buffers"][0]["uri"] = bin_path.name
        elif blob:
            doc["buffers"][0]["uri"] = "data:application/octet-stream;base64," + base64.b64encode(blob).decode()
        path.write_text(json.dumps(doc, indent=1))
        return path


def trs_node(translation=None, rotation=None, scale=None, **kw):
    n = dict(kw)
    for key, v in (("translation", translation), ("rotation", rotation), ("scale", scale)):
        if v is not None:
            n[key] = [float(x) for x in v]
    return n


def matrix_node(matrix, **kw):
    """matrix: 4x4 acting on column vectors; stored column-major."""
    return dict(kw, matrix=[float(x) for x in np.asarray(matrix, np.float64).reshape(4, 4).T.reshape(-1)])


def add_animation(w: Writer, channels, name="anim") -> int:
    """channels: (node, path, times, values, interpolation); values [keys, width] (CUBICSPLINE: [keys, 3, width])."""
    a = {"name": name, "samplers": [], "channels": []}
    for node, path, times, values, interp in channels:
        v = np.asarray(values, np.float64)
        width = 1 if path == "weights" else v.shape[-1]
        a["samplers"].append({"input": w.accessor(np.asarray(times, np.float64)),
                              "output": w.accessor(v.reshape(-1, width)), "interpolation": interp})
        a["channels"].append({"sampler": len(a["samplers"]) - 1, "target": {"node": node, "path": path}})
    return w.add("animations", a)
