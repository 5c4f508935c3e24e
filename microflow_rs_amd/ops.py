"""microflow::ops -- the reference's operator functions (src/ops/mod.rs) with the same
names, argument order and meaning, executed by the HIP kernels behind the C ABI.

    fully_connected(input, weights, output_scale, output_zero_point, options, constants)
    conv_2d(input, filters, output_scale, output_zero_point, options, constants, output_shape)
    depthwise_conv_2d(input, weights, output_scale, output_zero_point, options, constants, output_shape)
    average_pool_2d(input, filter_shape, output_scale, output_zero_point, options, constants, output_shape)
    max_pool_2d(input, filter_shape, output_scale, output_zero_point, options, constants, output_shape)   (not in the reference)
    add(a, b, output_scale, output_zero_point, options, constants)                                        (not in the reference)
    concatenation(a, b, output_scale, output_zero_point, options, constants)                              (not in the reference)
    pad(input, pads)                                                                                      (not in the reference)
    softmax(input, output_scale, output_zero_point)
    reshape(input, output_shape)

Differences forced by the language: output shapes are const generics in Rust and an
explicit `output_shape=(rows, cols)` here; buffers are row-major / NHWC arrays
(include/microflow_amd.h).  A leading batch of independent inferences is allowed on
every operator (`input.buffer` may have one extra leading dimension).
"""
import ctypes as C
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib
from .tensor import FusedActivation, Tensor2D, Tensor4D, TensorViewPadding


@dataclass
class FullyConnectedOptions:              # src/ops/fully_connected.rs:9-11
    fused_activation: FusedActivation = FusedActivation.NONE


@dataclass
class Conv2DOptions:                      # src/ops/conv_2d.rs:11-15
    fused_activation: FusedActivation = FusedActivation.NONE
    view_padding: TensorViewPadding = TensorViewPadding.SAME
    strides: Tuple[int, int] = (1, 1)


@dataclass
class DepthwiseConv2DOptions:             # src/ops/depthwise_conv_2d.rs:11-15
    fused_activation: FusedActivation = FusedActivation.NONE
    view_padding: TensorViewPadding = TensorViewPadding.SAME
    strides: Tuple[int, int] = (1, 1)


@dataclass
class AveragePool2DOptions:               # src/ops/average_pool_2d.rs:12-16
    fused_activation: FusedActivation = FusedActivation.NONE
    view_padding: TensorViewPadding = TensorViewPadding.SAME
    strides: Tuple[int, int] = (1, 1)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _lib.MicroflowError(_lib.MF_ERR_NO_DEVICE,
                                  "no GPU visible: microflow ops have no CPU fallback")
    return torch


def _host(a, dtype):
    return np.ascontiguousarray(np.asarray(a, dtype=dtype))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _elem(a):
    """Element type T (src/quantize.rs:32-53) of a buffer: np.uint8 -> u8, everything else i8."""
    dt = getattr(a, "dtype", None)
    if dt is None:
        return np.int8
    try:
        import torch
        if dt == torch.uint8:
            return np.uint8
    except ImportError:
        pass
    return np.uint8 if dt == np.uint8 else np.int8


def _fn(name, dtype):
    return getattr(_lib.lib(), name + ("_u8" if dtype == np.uint8 else ""))


class PreparedOp:
    """A prepared operator (mf_op): weights + folded constants resident in HBM."""

    def __init__(self, handle, in_tail, out_tail, dtype=np.int8, binary=False, in2_tail=None):
        self._h = handle
        self.binary = binary   # an ADD or a CONCATENATION: two inputs (mf_op_run2)
        self.in2_tail = None if in2_tail is None else tuple(in2_tail)   # the second input's shape where it differs (CONCATENATION)
        self.in_tail, self.out_tail = tuple(in_tail), tuple(out_tail)
        self.dtype = dtype

    @property
    def kernel(self):
        return _lib.lib().mf_op_kernel_name(self._h).decode()

    def set_generic(self, generic=True):
        _lib.check(_lib.lib().mf_op_set_generic(self._h, int(generic)))
        return self

    def _stage(self, x):
        torch = _torch()
        is_np = not isinstance(x, torch.Tensor)
        tdt = torch.uint8 if self.dtype == np.uint8 else torch.int8
        if is_np and isinstance(x, np.ndarray) and x.dtype.kind in "iu" and x.dtype.itemsize == 1 \
                and x.dtype != self.dtype:
            raise TypeError("%s tensor expected" % np.dtype(self.dtype).name)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=self.dtype)).cuda() if is_np else x.contiguous()
        if xt.dtype != tdt:
            raise TypeError("%s tensor expected" % np.dtype(self.dtype).name)
        return xt, is_np, tdt

    def __call__(self, x, y=None):
        """x: numpy (host) or torch cuda tensor of the operator's element type (int8 / uint8),
        shape [..batch] + in_tail.  An ADD takes two of them, of one shape: x is operand a, y operand b; a CONCATENATION's y
        has shape [..batch] + in2_tail."""
        torch = _torch()
        if self.binary != (y is not None):
            raise TypeError("the operator takes %s" % ("two inputs" if self.binary else "one input"))
        xt, is_np, tdt = self._stage(x)
        if self.binary:
            yt = self._stage(y)[0]
            if self.in2_tail is None and (tuple(yt.shape) != tuple(xt.shape) or yt.device != xt.device):
                raise ValueError("the two inputs of an ADD must have one shape and one device")
        in_elems = int(np.prod(self.in_tail))
        if self.binary and self.in2_tail is not None and (
                yt.device != xt.device or yt.numel() * in_elems != xt.numel() * int(np.prod(self.in2_tail))):
            raise ValueError("the two inputs of a CONCATENATION must hold the same rows on one device")
        if xt.numel() % in_elems:
            raise ValueError("input size %d is not a multiple of %d" % (xt.numel(), in_elems))
        batch = xt.numel() // in_elems
        nt = len(self.in_tail)
        if xt.dim() >= nt and tuple(xt.shape[-nt:]) == self.in_tail:
            lead = tuple(xt.shape[:-nt])   # [..batch dims] + operator shape
        else:
            lead = (batch,)
        out = torch.empty(lead + self.out_tail, dtype=tdt, device=xt.device)
        stream = torch.cuda.current_stream(xt.device).cuda_stream
        if self.binary:
            _lib.check(_lib.lib().mf_op_run2(self._h, xt.data_ptr(), yt.data_ptr(), batch, out.data_ptr(), stream))
        else:
            _lib.check(_lib.lib().mf_op_run(self._h, xt.data_ptr(), batch, out.data_ptr(), stream))
        if is_np:
            return out.cpu().numpy()
        return out

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().mf_op_destroy(h)
            except Exception:  # noqa: BLE001
                pass


def _device():
    torch = _torch()
    return torch.cuda.current_device()


def prepare_fully_connected(M, weights_nk, weights_zero_point, output_scale, output_zero_point,
                            options, constants):
    dt = _elem(weights_nk)
    w = _host(weights_nk, dt)
    N, K = w.shape
    c0, c1, c2, c3 = constants
    c0, c2 = _host(np.reshape(c0, -1), np.float32), _host(np.reshape(c2, -1), np.int32)
    h = C.c_void_p()
    _lib.check(_fn("mf_fully_connected_create", dt)(
        _device(), M, K, N, _ptr(w), int(weights_zero_point), float(output_scale),
        int(output_zero_point), int(options.fused_activation), _ptr(c0), float(c1), _ptr(c2),
        int(c3), C.byref(h)))
    return PreparedOp(h, (M, K), (M, N), dt)


def fully_connected(input: Tensor2D, weights: Tensor2D, output_scale, output_zero_point,
                    options: FullyConnectedOptions, constants) -> Tensor2D:
    """microflow::ops::fully_connected (src/ops/fully_connected.rs:24-41).
    `weights.buffer` is K x N like the reference's Tensor2D<T, INPUT_COLS, WEIGHTS_COLS>."""
    w_kn = np.asarray(weights.buffer, dtype=_elem(weights.buffer))
    M = int(input.buffer.shape[-2])
    op = prepare_fully_connected(M, w_kn.T, weights.zero_point[0], output_scale[0],
                                 output_zero_point[0], options, constants)
    return Tensor2D(op(input.buffer), list(output_scale), list(output_zero_point))


def prepare_conv_2d(in_hwc, filters, filters_zero_point, input_zero_point, output_scale,
                    output_zero_point, options, constants, out_hw):
    dt = _elem(filters)
    f = _host(filters, dt)
    N, KH, KW, Cc = f.shape
    H, W, C_in = in_hwc
    if C_in != Cc:
        raise ValueError("filter channels != input channels")
    fzp = _host(np.reshape(filters_zero_point, -1), dt)
    c0, c1 = (_host(np.reshape(c, -1), np.float32) for c in constants)
    h = C.c_void_p()
    _lib.check(_fn("mf_conv_2d_create", dt)(
        _device(), H, W, Cc, N, KH, KW, _ptr(f), _ptr(fzp), fzp.size, int(input_zero_point),
        float(output_scale), int(output_zero_point), int(options.fused_activation),
        int(options.view_padding), options.strides[0], options.strides[1], out_hw[0], out_hw[1],
        _ptr(c0), _ptr(c1), c1.size, C.byref(h)))
    return PreparedOp(h, (H, W, Cc), (out_hw[0], out_hw[1], N), dt)


def conv_2d(input: Tensor4D, filters: Tensor4D, output_scale, output_zero_point,
            options: Conv2DOptions, constants, output_shape) -> Tensor4D:
    """microflow::ops::conv_2d (src/ops/conv_2d.rs:28-49)."""
    shp = tuple(input.buffer.shape)
    op = prepare_conv_2d(shp[-3:], filters.buffer, filters.zero_point, input.zero_point[0],
                         output_scale[0], output_zero_point[0], options, constants, output_shape)
    return Tensor4D(op(input.buffer), list(output_scale), list(output_zero_point))


def prepare_depthwise_conv_2d(in_hwc, weights, weights_zero_point, input_zero_point, output_scale,
                              output_zero_point, options, constants, out_hw):
    dt = _elem(weights)
    w = _host(weights, dt)
    if w.ndim == 4:
        w = w[0]
    KH, KW, WC = w.shape
    H, W, Cin = in_hwc
    wzp = _host(np.reshape(weights_zero_point, -1), dt)
    c0, c1 = (_host(np.reshape(c, -1), np.float32) for c in constants)
    h = C.c_void_p()
    _lib.check(_fn("mf_depthwise_conv_2d_create", dt)(
        _device(), H, W, Cin, KH, KW, WC, _ptr(w), _ptr(wzp), wzp.size, int(input_zero_point),
        float(output_scale), int(output_zero_point), int(options.fused_activation),
        int(options.view_padding), options.strides[0], options.strides[1], out_hw[0], out_hw[1],
        _ptr(c0), _ptr(c1), c1.size, C.byref(h)))
    return PreparedOp(h, (H, W, Cin), (out_hw[0], out_hw[1], WC), dt)


def depthwise_conv_2d(input: Tensor4D, weights: Tensor4D, output_scale, output_zero_point,
                      options: DepthwiseConv2DOptions, constants, output_shape) -> Tensor4D:
    """microflow::ops::depthwise_conv_2d (src/ops/depthwise_conv_2d.rs:28-49)."""
    shp = tuple(input.buffer.shape)
    op = prepare_depthwise_conv_2d(shp[-3:], weights.buffer, weights.zero_point,
                                   input.zero_point[0], output_scale[0], output_zero_point[0],
                                   options, constants, output_shape)
    return Tensor4D(op(input.buffer), list(output_scale), list(output_zero_point))


def prepare_average_pool_2d(in_hwc, filter_shape, output_scale, output_zero_point, options,
                            constants, out_hw, dtype=np.int8):
    H, W, Cc = in_hwc
    h = C.c_void_p()
    _lib.check(_fn("mf_average_pool_2d_create", dtype)(
        _device(), H, W, Cc, filter_shape[0], filter_shape[1], float(output_scale),
        int(output_zero_point), int(options.fused_activation), int(options.view_padding),
        options.strides[0], options.strides[1], out_hw[0], out_hw[1], float(constants[0]),
        float(constants[1]), C.byref(h)))
    return PreparedOp(h, (H, W, Cc), (out_hw[0], out_hw[1], Cc), dtype)


def average_pool_2d(input: Tensor4D, filter_shape, output_scale, output_zero_point,
                    options: AveragePool2DOptions, constants, output_shape) -> Tensor4D:
    """microflow::ops::average_pool_2d (src/ops/average_pool_2d.rs:29-45)."""
    shp = tuple(input.buffer.shape)
    op = prepare_average_pool_2d(shp[-3:], filter_shape, output_scale[0], output_zero_point[0],
                                 options, constants, output_shape, dtype=_elem(input.buffer))
    return Tensor4D(op(input.buffer), list(output_scale), list(output_zero_point))


MaxPool2DOptions = AveragePool2DOptions


def prepare_max_pool_2d(in_hwc, filter_shape, output_scale, output_zero_point, options,
                        constants, out_hw, dtype=np.int8):
    H, W, Cc = in_hwc
    h = C.c_void_p()
    _lib.check(_fn("mf_max_pool_2d_create", dtype)(
        _device(), H, W, Cc, filter_shape[0], filter_shape[1], float(output_scale),
        int(output_zero_point), int(options.fused_activation), int(options.view_padding),
        options.strides[0], options.strides[1], out_hw[0], out_hw[1], float(constants[0]),
        float(constants[1]), C.byref(h)))
    return PreparedOp(h, (H, W, Cc), (out_hw[0], out_hw[1], Cc), dtype)


def max_pool_2d(input: Tensor4D, filter_shape, output_scale, output_zero_point,
                options: MaxPool2DOptions, constants, output_shape) -> Tensor4D:
    """MaxPool2D (TFLite builtin 17; the reference has none): average_pool_2d's window placement and constants, the max over the
    in-bounds taps, then roundf(c0 * f32(max) + c1) and the fused activation (include/microflow_amd.h)."""
    shp = tuple(input.buffer.shape)
    op = prepare_max_pool_2d(shp[-3:], filter_shape, output_scale[0], output_zero_point[0],
                             options, constants, output_shape, dtype=_elem(input.buffer))
    return Tensor4D(op(input.buffer), list(output_scale), list(output_zero_point))


@dataclass
class AddOptions:                         # (not in the reference) tflite.fbs AddOptions
    fused_activation: FusedActivation = FusedActivation.NONE


def preprocess_add(a_scale, b_scale, output_scale):
    """(ca, cb) = (a_scale / output_scale, b_scale / output_scale) in f32, as the library's host computes them."""
    ca, cb = C.c_float(0), C.c_float(0)
    _lib.check(_lib.lib().mf_preprocess_add(float(a_scale), float(b_scale), float(output_scale), C.byref(ca), C.byref(cb)))
    return np.float32(ca.value), np.float32(cb.value)


def prepare_add(elems_or_shape, a_q, b_q, out_q, options, constants=None, dtype=np.int8):
    """a_q, b_q, out_q: (scale, zero_point) of the two operands and the output; constants: (ca, cb), computed when None."""
    tail = (int(elems_or_shape),) if np.isscalar(elems_or_shape) else tuple(int(d) for d in elems_or_shape)
    if constants is None:
        constants = preprocess_add(a_q[0], b_q[0], out_q[0])
    h = C.c_void_p()
    _lib.check(_fn("mf_add_create", dtype)(
        _device(), int(np.prod(tail)), float(a_q[0]), int(a_q[1]), float(b_q[0]), int(b_q[1]), float(out_q[0]), int(out_q[1]),
        int(options.fused_activation), float(constants[0]), float(constants[1]), C.byref(h)))
    return PreparedOp(h, tail, tail, dtype, binary=True)


def add(a, b, output_scale, output_zero_point, options: AddOptions, constants=None):
    """ADD (TFLite builtin 0; the reference has none) of two tensors of one shape and element type, per-tensor quantisation:
    y = T::from(roundf((f32(zo) + ca * f32(a - za)) + cb * f32(b - zb))), every step rounded to f32, then the fused activation
    (include/microflow_amd.h).  The operand order is kept."""
    shp = tuple(a.buffer.shape)
    tail = shp[-3:] if len(shp) >= 3 else shp[-2:]
    op = prepare_add(tail, (a.scale[0], a.zero_point[0]), (b.scale[0], b.zero_point[0]),
                     (output_scale[0], output_zero_point[0]), options, constants, dtype=_elem(a.buffer))
    return type(a)(op(a.buffer, b.buffer), list(output_scale), list(output_zero_point))


@dataclass
class ConcatenationOptions:               # (not in the reference) tflite.fbs ConcatenationOptions; no fused activation
    axis: int = -1


def preprocess_concatenation(a_scale, b_scale, output_scale):
    """(ca, cb) = (a_scale / output_scale, b_scale / output_scale) in f32, as the library's host computes them."""
    ca, cb = C.c_float(0), C.c_float(0)
    _lib.check(_lib.lib().mf_preprocess_concatenation(float(a_scale), float(b_scale), float(output_scale), C.byref(ca), C.byref(cb)))
    return np.float32(ca.value), np.float32(cb.value)


def prepare_concatenation(rows_or_shape, Ca, Cb, a_q, b_q, out_q, constants=None, dtype=np.int8):
    """rows_or_shape: the axes in front of the last one (their product is `rows`); a_q, b_q, out_q: (scale, zero_point) of the two
    inputs and the output; constants: (ca, cb), computed when None."""
    lead = (int(rows_or_shape),) if np.isscalar(rows_or_shape) else tuple(int(d) for d in rows_or_shape)
    if constants is None:
        constants = preprocess_concatenation(a_q[0], b_q[0], out_q[0])
    h = C.c_void_p()
    _lib.check(_fn("mf_concatenation_create", dtype)(
        _device(), int(np.prod(lead)), int(Ca), int(Cb), float(a_q[0]), int(a_q[1]), float(b_q[0]), int(b_q[1]), float(out_q[0]),
        int(out_q[1]), float(constants[0]), float(constants[1]), C.byref(h)))
    return PreparedOp(h, lead + (int(Ca),), lead + (int(Ca) + int(Cb),), dtype, binary=True, in2_tail=lead + (int(Cb),))


def concatenation(a, b, output_scale, output_zero_point, options: ConcatenationOptions = None, constants=None):
    """CONCATENATION (TFLite builtin 2; the reference has none) of two tensors along the last axis, per-tensor quantisation: every
    element of input i becomes T::from(roundf(f32(zo) + c_i * f32(x - z_i))), every step rounded to f32 (include/microflow_amd.h);
    a slice whose quantisation is the output's is copied.  The operand order is kept."""
    shp_a, shp_b = tuple(a.buffer.shape), tuple(b.buffer.shape)
    nd = 3 if isinstance(a, Tensor4D) else 2   # axes of one inference in the buffer: H, W, C or rows, cols
    axis = -1 if options is None else int(options.axis)
    if axis not in (-1, 3 if isinstance(a, Tensor4D) else 1):   # (counted in the tensor's own rank: [1][H][W][C] or [rows][cols])
        raise ValueError("concatenation: only the last axis is supported")
    if shp_a[:-1] != shp_b[:-1]:
        raise ValueError("concatenation: the inputs differ in another dimension than the axis")
    op = prepare_concatenation(shp_a[-nd:-1], shp_a[-1], shp_b[-1], (a.scale[0], a.zero_point[0]), (b.scale[0], b.zero_point[0]),
                               (output_scale[0], output_zero_point[0]), constants, dtype=_elem(a.buffer))
    return type(a)(op(a.buffer, b.buffer), list(output_scale), list(output_zero_point))


def prepare_pad(in_hwc, pads, zero_point, dtype=np.int8):
    """pads: ((top, bottom), (left, right)) new rows / columns around the H x W x C image, each new element zero_point."""
    H, W, Cc = (int(d) for d in in_hwc)
    (t, b), (l, r) = ((int(v) for v in p) for p in pads)
    h = C.c_void_p()
    _lib.check(_fn("mf_pad_create", dtype)(_device(), H, W, Cc, t, b, l, r, int(zero_point), C.byref(h)))
    return PreparedOp(h, (H, W, Cc), (H + t + b, W + l + r, Cc), dtype)


def pad(input: Tensor4D, pads) -> Tensor4D:
    """PAD (TFLite builtin 34; the reference has none) in H and W: the tensor with new rows and columns of its own zero point around
    every image; scale and zero point stay (include/microflow_amd.h).  MEAN over H and W needs no function of its own: it is
    average_pool_2d with the whole image as filter."""
    shp = tuple(input.buffer.shape)
    op = prepare_pad(shp[-3:], pads, input.zero_point[0], dtype=_elem(input.buffer))
    return Tensor4D(op(input.buffer), list(input.scale), list(input.zero_point))


def prepare_softmax(rows, cols, input_scale, output_scale, output_zero_point, dtype=np.int8):
    h = C.c_void_p()
    _lib.check(_fn("mf_softmax_create", dtype)(_device(), rows, cols, float(input_scale),
                                               float(output_scale), int(output_zero_point),
                                               C.byref(h)))
    return PreparedOp(h, (rows, cols), (rows, cols), dtype)


def softmax(input: Tensor2D, output_scale, output_zero_point) -> Tensor2D:
    """microflow::ops::softmax (src/ops/softmax.rs:15-19)."""
    rows, cols = input.buffer.shape[-2:]
    op = prepare_softmax(int(rows), int(cols), input.scale[0], output_scale[0], output_zero_point[0],
                         dtype=_elem(input.buffer))
    return Tensor2D(op(input.buffer), list(output_scale), list(output_zero_point))


def reshape(input, output_shape):
    """microflow::ops::reshape (src/ops/reshape.rs:3-8): the 2D<->4D conversions of
    src/tensor.rs:103-141 keep logical NHWC order, i.e. a plain reshape of row-major memory."""
    buf = input.buffer.reshape(tuple(output_shape))
    cls = Tensor2D if len(output_shape) == 2 else Tensor4D
    return cls(buf, list(input.scale), list(input.zero_point))


def quantize(x, scale, zero_point, dtype=np.int8):
    """Tensor{2D,4D}::quantize (src/tensor.rs:80-86,246-256) on the device; dtype = T."""
    torch = _torch()
    is_np = not isinstance(x, torch.Tensor)
    xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda() if is_np else x.contiguous()
    out = torch.empty(xt.shape, dtype=torch.uint8 if dtype == np.uint8 else torch.int8, device=xt.device)
    _lib.check(_fn("mf_quantize", dtype)(xt.device.index or 0, xt.data_ptr(), xt.numel(), float(scale),
                                      int(zero_point), out.data_ptr(),
                                      torch.cuda.current_stream(xt.device).cuda_stream))
    return out.cpu().numpy() if is_np else out


def dequantize(q, scale, zero_point):
    """Tensor{2D,4D}::dequantize (src/tensor.rs:89-92,259-262) on the device."""
    torch = _torch()
    is_np = not isinstance(q, torch.Tensor)
    dt = _elem(q)
    qt = torch.as_tensor(np.ascontiguousarray(q, dtype=dt)).cuda() if is_np else q.contiguous()
    out = torch.empty(qt.shape, dtype=torch.float32, device=qt.device)
    _lib.check(_fn("mf_dequantize", dt)(qt.device.index or 0, qt.data_ptr(), qt.numel(),
                                        float(scale), int(zero_point), out.data_ptr(),
                                        torch.cuda.current_stream(qt.device).cuda_stream))
    return out.cpu().numpy() if is_np else out
