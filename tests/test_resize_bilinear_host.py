"""RESIZE_BILINEAR without a GPU: the loader reads builtin 23 with half-pixel centres, reports the kind, the name and the factors, loads
the bilinear decoder models and refuses what the contract (include/microflow_amd.h: mf_resize_bilinear_create) refuses, each with its
status and reason."""
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


def test_builtin_23_loads_and_reports_kind_name_and_factors():
    import microflow_rs_amd as mf
    m = _load([tw._resize_layer((4, 6, 8), Q, (3, 2), bilinear=True), tw._conv_layer(np.random.default_rng(1), (12, 12, 8), Q, False, 8, 3, 1)])
    assert m.op(0)["kind"] == 23 == mf._lib.MF_OP_RESIZE_BILINEAR and m.op(0)["name"] == "resize_bilinear"
    assert m.op(0)["out_shape"] == (1, 12, 12, 8) and m.op_upsample(0) == (3, 2)
    with pytest.raises(mf._lib.MicroflowError):
        m.op_upsample(1)


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("name", ["upsample_autoencoder", "unet1", "seg_head"])
def test_the_bilinear_models_load(name, u8):
    import microflow_rs_amd as mf
    elem = tw.UINT8 if u8 else tw.INT8
    if name == "seg_head":
        m = mf.model(tw.seg_head(np.random.default_rng(2), (16, 16, 4), (8, 16), 5, elem=elem))
        want, out, last = 1, (1, 16, 16, 5), True
    else:
        m = mf.model(getattr(tw, name)(np.random.default_rng(2), (16, 16, 4), (8, 16), elem=elem, interpolation="bilinear"))
        want, out, last = (2 if name == "upsample_autoencoder" else 1), (1, 16, 16, 4), False
    kinds = [m.op(i)["name"] for i in range(m.num_ops)]
    assert kinds.count("resize_bilinear") == want and "resize_nearest_neighbor" not in kinds and m.output_shape == out, kinds
    assert (kinds[-1] == "resize_bilinear") == last
    assert all(m.op_upsample(i) == ((4, 4) if last else (2, 2)) for i, k in enumerate(kinds) if k == "resize_bilinear")


R = tw._resize_layer((4, 6, 8), Q, (2, 2), bilinear=True)
REFUSALS = {
    "legacy":        (dict(R, half_pixel_centers=False), "UNSUPPORTED", "23 (RESIZE_BILINEAR: half_pixel_centers = false)"),
    "ratio":         (dict(R, out_shape=(1, 6, 12, 8)), "UNSUPPORTED", "23 (RESIZE_BILINEAR: a non-integer ratio)"),
    "align_corners": (dict(R, align_corners=True), "UNSUPPORTED", "23 (RESIZE_BILINEAR: align_corners = true)"),
    "size":          (dict(R, size_const=False), "UNSUPPORTED", "23 (RESIZE_BILINEAR: a non-constant size)"),
    "quant":         (dict(R, out_q=(0.06, -3)), "UNSUPPORTED", "23 (RESIZE_BILINEAR: input and output quantisation differ)"),
    "zero_point":    (dict(R, out_q=(0.05, 4)), "UNSUPPORTED", "23 (RESIZE_BILINEAR: input and output quantisation differ)"),
    "per_channel":   (dict(R, out_q=((0.05, 0.05), (-3, -3))), "UNSUPPORTED", "23 (RESIZE_BILINEAR: per-channel quantisation on an operand)"),
    "mixed":         (dict(R, out_type=tw.UINT8), "UNSUPPORTED", "23 (RESIZE_BILINEAR: mixed element types)"),
    "batch":         (dict(R, out_shape=(2, 8, 12, 8)), "UNSUPPORTED", "23 (RESIZE_BILINEAR: tensor batch must be 1)"),
    "contradiction": (dict(R, size=(8, 14)), "INVALID_MODEL", "RESIZE_BILINEAR size disagrees with the output tensor's shape"),
}


@pytest.mark.parametrize("case", REFUSALS, ids=list(REFUSALS))
def test_refusals(case):
    from microflow_rs_amd import _lib
    layer, status, text = REFUSALS[case]
    with pytest.raises(_lib.MicroflowError) as e:   # (a convolution behind it: the model's output keeps the input's type)
        _load([layer, tw._conv_layer(np.random.default_rng(1), (8, 12, 8), Q, False, 8, 3, 1)])
    assert e.value.status == getattr(_lib, "MF_ERR_" + status) and text in e.value.message, e.value
    assert status != "UNSUPPORTED" or e.value.message.startswith("unsupported operator: "), e.value.message
