"""rsd.convnet -- the ConvolutionalNet pass's networks (rsd_convnet_*, include/rsd_graph.h).

A net is a list of layers; layer l holds `weights` [slices][K][K][Cin][Cout] (axis 1 is the X offset and axis 2 the Y
offset of the tap: the reference's order, the transpose of Keras') and `bias` [slices][Cout] or None.  The reference
keeps one net per array slice in a directory, <slice>_weight_<l>.npy ([K][K][Cin][Cout]) and <slice>_bias_<l>.npy:

    save_dir(dir, layers)          write that layout with numpy
    ConvNet.from_dir(dir, slices)  load it through librsd: every value is rounded to the 6 significant digits the
                                   reference prints into its shader text
    ConvNet.from_arrays(layers)    the arrays as they are
"""
import ctypes as C
from pathlib import Path

import numpy as np

from . import abi


def _as_layers(layers):
    """[(weights [S][K][K][Cin][Cout] float32, bias [S][Cout] float32 or None)] from tuples or dicts."""
    out = []
    for layer in layers:
        w, b = (layer["weights"], layer.get("bias")) if isinstance(layer, dict) else layer
        w = np.ascontiguousarray(w, np.float32)
        if w.ndim != 5:
            raise ValueError("weights must be [slices][K][K][Cin][Cout]")
        if w.shape[1] != w.shape[2]:
            raise ValueError("non-square kernels are not supported")
        if b is not None:
            b = np.ascontiguousarray(b, np.float32)
            if b.shape != (w.shape[0], w.shape[4]):
                raise ValueError("bias must be [slices][Cout]")
        out.append((w, b))
    if not out or len({w.shape[0] for w, _ in out}) != 1:
        raise ValueError("a net needs at least one layer, and every layer the same slice count")
    return out


def save_dir(directory, layers):
    """Write `layers` (see the module text) into `directory` in the reference's file layout."""
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    for l, (w, b) in enumerate(_as_layers(layers)):
        for s in range(w.shape[0]):
            np.save(directory / f"{s}_weight_{l}.npy", w[s])
            if b is not None:
                np.save(directory / f"{s}_bias_{l}.npy", b[s])


class ConvNet:
    """A loaded net (rsd_convnet).  Host memory until its first run on a device."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)
        info = abi.ConvNetInfo()
        abi.check(abi.lib().rsd_convnet_get_info(self.h, C.byref(info)), "rsd_convnet_get_info")
        self.layers, self.slices, self.radius, self.fused = info.layers, info.slices, info.radius, bool(info.fused)
        self.kernel = list(info.kernel[:info.layers])
        self.channels_in = list(info.channels_in[:info.layers])
        self.channels_out = list(info.channels_out[:info.layers])

    @classmethod
    def from_dir(cls, directory, slices=16):
        h = C.c_void_p()
        abi.check(abi.lib().rsd_convnet_load_dir(str(directory).encode(), int(slices), C.byref(h)), "rsd_convnet_load_dir")
        return cls(h.value)

    @classmethod
    def from_arrays(cls, layers):
        arrays = _as_layers(layers)
        desc = (abi.ConvNetLayer * len(arrays))()
        for d, (w, b) in zip(desc, arrays):
            d.kernel, d.channels_in, d.channels_out = w.shape[1], w.shape[3], w.shape[4]
            d.weights = w.ctypes.data
            d.bias = b.ctypes.data if b is not None else None
        h = C.c_void_p()
        abi.check(abi.lib().rsd_convnet_create(desc, len(arrays), arrays[0][0].shape[0], C.byref(h)), "rsd_convnet_create")
        return cls(h.value)  # librsd copied the arrays

    def scratch_bytes(self, params) -> int:
        return int(abi.lib().rsd_convnet_scratch_bytes(self.h, C.byref(params)))

    def scratch_layout(self, params):
        """[(byte offset, (slices, Cout, h, w))] of the layers' activations in the scratch of a per-layer run."""
        qw, qh = ((params.width + 3) // 4, (params.height + 3) // 4) if params.layers == 16 else (params.width, params.height)
        elem = {abi.CONVNET_FLOAT: 4, abi.CONVNET_HALF: 2, abi.CONVNET_UNORM: 1}[params.precision]
        out, off = [], 0
        for cout in self.channels_out[:-1]:
            out.append((off, (self.slices, cout, qh, qw)))
            off += (self.slices * cout * qh * qw * elem + 255) // 256 * 256
        return out

    def run(self, params, bright, dark, importance, depth, scratch, out, stream=None):
        """rsd_convnet_run on device pointers (ints or None)."""
        abi.check(abi.lib().rsd_convnet_run(self.h, C.byref(params), bright, dark, importance, depth, scratch, out, stream),
                  "rsd_convnet_run")

    def close(self):
        if self.h:
            abi.lib().rsd_convnet_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
