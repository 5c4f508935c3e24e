"""RESIZE_NEAREST_NEIGHBOR without a GPU: the loader reads builtin 97, reports the kind and the factors, loads the UpSampling2D models and
refuses what the contract (include/microflow_amd.h: mf_resize_nearest_create) refuses, each with its status and reason."""
import os
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

Q = (0.05, -3)


def _load(layers, shape=(1, 4, 6, 8), elem=tw.INT8):
    return __import__("microflow_rs_amd").model(tw.build_model(shape, Q, layers, elem))


def test_builtin_97_loads_and_reports_kind_and_factors():
    import microflow_rs_amd as mf
    m = _load([tw._resize_layer((4, 6, 8), Q, (3, 2)), tw._conv_layer(np.random.default_rng(1), (12, 12, 8), Q, False, 8, 3, 1)])
    assert m.op(0)["kind"] == 97 == mf._lib.MF_OP_RESIZE_NEAREST_NEIGHBOR and m.op(0)["name"] == "resize_nearest_neighbor"
    assert m.op(0)["out_shape"] == (1, 12, 12, 8) and m.op_upsample(0) == (3, 2)
    with pytest.raises(mf._lib.MicroflowError):
        m.op_upsample(1)
    assert _load([dict(tw._resize_layer((4, 6, 8), Q, (2, 2)), half_pixel_centers=True)]).op_upsample(0) == (2, 2)


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("name", ["upsample_autoencoder", "unet1"])
def test_the_upsampling_models_load(name, u8):
    import microflow_rs_amd as mf
    m = mf.model(getattr(tw, name)(np.random.default_rng(2), (16, 16, 4), (8, 16), elem=tw.UINT8 if u8 else tw.INT8))
    kinds = [m.op(i)["name"] for i in range(m.num_ops)]
    assert kinds.count("resize_nearest_neighbor") == (2 if name == "upsample_autoencoder" else 1) and m.output_shape == (1, 16, 16, 4), kinds
    assert all(m.op_upsample(i) == (2, 2) for i, k in enumerate(kinds) if k.startswith("resize"))


R = tw._resize_layer((4, 6, 8), Q, (2, 2))
REFUSALS = {
    "ratio":         (dict(R, out_shape=(1, 6, 12, 8)), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: a non-integer ratio)"),
    "align_corners": (dict(R, align_corners=True), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: align_corners = true)"),
    "size":          (dict(R, size_const=False), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: a non-constant size)"),
    "quant":         (dict(R, out_q=(0.06, -3)), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: input and output quantisation differ)"),
    "zero_point":    (dict(R, out_q=(0.05, 4)), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: input and output quantisation differ)"),
    "per_channel":   (dict(R, out_q=((0.05, 0.05), (-3, -3))), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: per-channel quantisation on an operand)"),
    "mixed":         (dict(R, out_type=tw.UINT8), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: mixed element types)"),
    "batch":         (dict(R, out_shape=(2, 8, 12, 8)), "UNSUPPORTED", "97 (RESIZE_NEAREST_NEIGHBOR: tensor batch must be 1)"),
    "contradiction": (dict(R, size=(8, 14)), "INVALID_MODEL", "RESIZE_NEAREST_NEIGHBOR size disagrees with the output tensor's shape"),
    "bilinear":      (dict(R, code="resize_bilinear"), "UNSUPPORTED", "unsupported operator: 23 (RESIZE_BILINEAR"),
}


@pytest.mark.parametrize("case", REFUSALS, ids=list(REFUSALS))
def test_refusals(case):
    from microflow_rs_amd import _lib
    layer, status, text = REFUSALS[case]
    with pytest.raises(_lib.MicroflowError) as e:   # (a convolution behind it: the model's output keeps the input's type)
        _load([layer, tw._conv_layer(np.random.default_rng(1), (8, 12, 8), Q, False, 8, 3, 1)])
    assert e.value.status == getattr(_lib, "MF_ERR_" + status) and text in e.value.message, e.value
    assert status != "UNSUPPORTED" or e.value.message.startswith("unsupported operator: "), e.value.message
