"""Sliding windows of a larger source (include/microflow_amd.h, section 5): the description, and the gather on its own.

A `Windows` says how the inferences of a batch lie inside something larger -- a spectrogram slid frame by frame, crops of camera
frames -- so that the source is handed over once, as it is; `Model.run_windows` / `predict_windows` / `predict_quantized_windows`
(model.py) run a model over them, `gather_windows` is the device kernel alone."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass(frozen=True)
class Windows:
    """mf_windows: per source ny = (src_rows - win_rows) // hop_rows + 1 by nx = (src_row_elems - win_row_elems) // hop_elems + 1
    windows; window (s * ny + iy) * nx + ix has element (r, e) at
    src[s * src_stride + (iy * hop_rows + r) * src_pitch + ix * hop_elems + e].  No padding."""
    src_rows: int
    src_row_elems: int
    win_rows: int
    win_row_elems: int
    hop_rows: int = 1
    hop_elems: int = 1
    src_pitch: int = None     # elements between source rows (default: src_row_elems)
    n_sources: int = 1
    src_stride: int = None    # elements between sources (default: src_rows * src_pitch)

    @classmethod
    def image(cls, src_hw, win_hw, channels, hop_px, n=1):
        """win_hw crops of n NHWC images of src_hw, every hop_px pixels (one int, or (rows, columns))"""
        hop_y, hop_x = (hop_px, hop_px) if np.isscalar(hop_px) else hop_px
        return cls(src_rows=int(src_hw[0]), src_row_elems=int(src_hw[1]) * int(channels), win_rows=int(win_hw[0]),
                   win_row_elems=int(win_hw[1]) * int(channels), hop_rows=int(hop_y), hop_elems=int(hop_x) * int(channels),
                   n_sources=int(n))

    @classmethod
    def frames(cls, n_frames, coeffs, win_frames, hop=1):
        """win_frames consecutive frames of a [n_frames][coeffs] signal, every hop frames"""
        return cls(src_rows=int(n_frames), src_row_elems=int(coeffs), win_rows=int(win_frames), win_row_elems=int(coeffs),
                   hop_rows=int(hop))

    @property
    def pitch(self):
        return self.src_row_elems if self.src_pitch is None else int(self.src_pitch)

    @property
    def stride(self):
        return self.src_rows * self.pitch if self.src_stride is None else int(self.src_stride)

    @property
    def window_elems(self):
        return self.win_rows * self.win_row_elems

    @property
    def source_elems(self):
        """elements from the first of source 0 to the last of the last source"""
        return (self.n_sources - 1) * self.stride + (self.src_rows - 1) * self.pitch + self.src_row_elems

    def desc(self):
        return _lib.WindowsDesc(self.n_sources, self.stride, self.src_rows, self.src_row_elems, self.pitch, self.win_rows,
                                self.win_row_elems, self.hop_rows, self.hop_elems)

    def counts(self):
        """(windows per source, windows in all), as mf_windows_count validates and counts them"""
        per, total = C.c_size_t(0), C.c_size_t(0)
        _lib.check(_lib.lib().mf_windows_count(C.byref(self.desc()), C.byref(per), C.byref(total)))
        return per.value, total.value

    @property
    def total(self):
        return self.counts()[1]

    def materialize(self, src):
        """the windows as a dense [total][window_elems] numpy array (host; what the device gather writes)"""
        a = np.asarray(src).reshape(-1)
        _, total = self.counts()
        ny = (self.src_rows - self.win_rows) // self.hop_rows + 1
        nx = (self.src_row_elems - self.win_row_elems) // self.hop_elems + 1
        if a.size < self.source_elems:
            raise ValueError("source has %d elements, the description needs %d" % (a.size, self.source_elems))
        it = a.itemsize
        v = np.lib.stride_tricks.as_strided(
            a, shape=(self.n_sources, ny, nx, self.win_rows, self.win_row_elems),
            strides=(self.stride * it, self.hop_rows * self.pitch * it, self.hop_elems * it, self.pitch * it, it), writeable=False)
        out = np.empty((total, self.window_elems), a.dtype)
        out.reshape(v.shape)[...] = v
        return out


def _range(windows, first, count):
    total = windows.counts()[1]
    first = int(first)
    count = total - first if count is None else int(count)
    if first < 0 or count < 0:
        raise ValueError("first and count must not be negative")
    return first, count


def gather_windows(src, windows, first=0, count=None, quantize=None, out=None):
    """Windows [first, first + count) of a cuda tensor as a dense [count][window_elems] tensor (mf_window_gather).
    src: int8 / uint8 at any byte offset, or -- with quantize=(scale, zero_point, np.int8 | np.uint8) -- float32, quantised on
    the way as mf_quantize[_u8] does (mf_window_gather_quantize[_u8])."""
    import torch
    if not (isinstance(src, torch.Tensor) and src.is_cuda):
        raise TypeError("gather_windows takes a cuda tensor (the entry point reads device memory)")
    first, count = _range(windows, first, count)
    x = src.contiguous().reshape(-1)
    if x.numel() < windows.source_elems:
        raise ValueError("source has %d elements, the description needs %d" % (x.numel(), windows.source_elems))
    dev = x.device.index or 0
    stream = torch.cuda.current_stream(x.device).cuda_stream
    L = _lib.lib()
    if quantize is None:
        if x.dtype not in (torch.int8, torch.uint8):
            raise TypeError("gather_windows takes int8 / uint8 (or float32 with quantize=), got %s" % x.dtype)
        odt = x.dtype
    else:
        if x.dtype != torch.float32:
            raise TypeError("quantize= takes a float32 source, got %s" % x.dtype)
        scale, zp, dt = quantize
        odt = torch.uint8 if np.dtype(dt) == np.uint8 else torch.int8
    if out is None:
        out = torch.empty((count, windows.window_elems), dtype=odt, device=x.device)
    elif not out.is_cuda or out.dtype != odt or out.numel() != count * windows.window_elems or not out.is_contiguous():
        raise ValueError("out= must be a contiguous cuda tensor of %d %s values" % (count * windows.window_elems, odt))
    d = windows.desc()
    if quantize is None:
        _lib.check(L.mf_window_gather(dev, x.data_ptr(), 1, C.byref(d), first, count, out.data_ptr(), stream))
    else:
        fn = L.mf_window_gather_quantize_u8 if odt == torch.uint8 else L.mf_window_gather_quantize
        _lib.check(fn(dev, x.data_ptr(), C.byref(d), first, count, float(scale), int(zp), out.data_ptr(), stream))
    return out
