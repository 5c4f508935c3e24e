"""PAD + VALID convolution as one launch where tests/test_gpu_pad_conv.py's 14 x 14 images at batch 5 do not reach: row
bands (NBANDS > 1: the band's first row is band BH sh - padt, rows outside the image are refilled every step, the last band is cut
by the rows that exist), more than one step per workgroup with a ragged last one, conv_rows_bytes with three channels at image and
step bases off the dword boundary, filter zero points in every Conv2D family, pads beyond the filter's reach (whole windows in
fill; top / left pads only), and conv_mm_rt's 1024-thread form.

The geometries and the plan numbers they rest on are tests/pad_cases.py's BANDED, SMALL and MANY_STEPS, pinned without a GPU by
tests/test_pad_conv_plan_host.py.  Every comparison is bit for bit against np.pad with the zero point + the CPU oracle's convolution
(tests/pad_ref.py)."""
import os
import sys

import numpy as np
import pytest

from tests import pad_cases as P
from tests import pad_ref
from tests.conftest import ROOT, ROUTING_SWITCHED
from tests.pad_run import ELEMS, FUSED, Prepared, check_every_way, names

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 0x5A
# the launch the PAD reports, by the planner the group routes to (P.PINNED)
KERNEL = {"conv_rows": "pad+conv_rows_lds", "conv_mm": "pad+conv_mm_rt", "conv_gemm": "pad+conv_gemm_rt", "dw_mm": "pad+dw_mm_rt<", "dw_gemm": "pad+dw_gemm_rt<"}


def check_kernel(name, got):
    """the PAD reports the one launch -- pad+ and the convolution's own kernel name on the unpadded image, its filter-zero-point and
    byte-form markers included -- and the convolution that it was swallowed"""
    if ROUTING_SWITCHED:
        return
    dw, H, W, C, K, S, pads, N, wz = P.EVERY[name]
    planner = P.PINNED[name][0]
    assert got[0].startswith(KERNEL[planner]) and got[1] == FUSED, (name, got)
    assert ("wzp" in got[0]) == wz, (name, got)
    if planner == "conv_rows":
        assert ("<bytes" in got[0]) == ((W * C) % 4 != 0), (name, got)   # rows that are not whole dwords: the conv_rows_bytes launch


_prepared = {}


def _case(O, name, ek):
    key = (name, ek)
    if key not in _prepared:
        elem, dt = ELEMS[ek]
        batch = 4 if name in P.BANDED else P.SMALL_BATCH.get(name, 5)
        _prepared[key] = Prepared(O, P.layers(P.EVERY[name], np.random.default_rng(17), elem), elem, dt, batch=batch, rows=True)
    return _prepared[key]


@pytest.mark.parametrize("ek", list(ELEMS))
@pytest.mark.parametrize("name", list(P.BANDED))
def test_banded_bytes_every_way(O, name, ek):
    """batch 4 -- all-minimum, all-maximum, edge-only, random -- under every way of running the model, and one more image whose rows
    are distinct constants through the default routing: a band whose first row is one off changes every output row of that one"""
    p = _case(O, name, ek)
    check_kernel(name, names(p.m))
    check_every_way(p)
    x = P.row_image(p.in_shape, p.in_q, p.dt)[None]
    want = p.ref(x.reshape(1, -1))[-1]
    got = np.asarray(p.m.run_quantized(x)).reshape(1, -1)
    assert np.array_equal(got, want), ("rows", names(p.m), int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    OH, OW = P.out_hw(P.EVERY[name])
    rows = want.reshape(OH, -1)
    assert len({r.tobytes() for r in rows}) > OH // 2    # (the image does tell output rows apart: the clamp does not flatten it)


@pytest.mark.parametrize("ek", list(ELEMS))
@pytest.mark.parametrize("name", list(P.SMALL))
def test_small_bytes_every_way(O, name, ek):
    """batch 5 (23 for the G = 7 shape: four steps, the last of two images), image 4 the row image"""
    p = _case(O, name, ek)
    check_kernel(name, names(p.m))
    check_every_way(p)


def _guarded(n, tdt):
    """-> (the whole buffer, its middle n bytes at a 16-byte-aligned address with GUARD sentinel bytes on either side)"""
    import torch
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=tdt, device="cuda")
    out = buf[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 0
    return buf, out


def _intact(buf, n):
    return bool((buf[:GUARD] == SENT).all().item() and (buf[GUARD + n:] == SENT).all().item())


MANY = [(name, ek) for name in P.MANY_STEPS for ek in ELEMS if ek == "i8" or P.PINNED[name][0] == "conv_rows"]


@pytest.mark.parametrize("name,ek", MANY, ids=["%s-%s" % c for c in MANY])
def test_many_steps_per_workgroup(O, name, ek):
    """more steps than twice the largest grid, a ragged last one (P.MANY_STEPS): the step loop and conv_rows_*'s fetch-ahead with the
    PAD's window placement.  The one launch against PAD, then the VALID convolution on the padded tensor, over the whole batch; the
    reference at the images on either side of a step boundary, in the middle and around the ragged last step; the output handed
    over inside a larger buffer whose guard bytes stay"""
    import torch
    import microflow_rs_amd as mf
    elem, dt = ELEMS[ek]
    G, nthr, batch = P.MANY_STEPS[name]
    r = batch % G
    in_shape, in_q, layers = P.layers(P.EVERY[name], np.random.default_rng(17), elem)
    m = mf.Model(tw.build_model(in_shape, in_q, layers, elem))
    m.prepare(batch)
    check_kernel(name, names(m))
    rng = np.random.default_rng(29)
    lo, hi = (0, 256) if dt == np.uint8 else (-128, 128)
    x = rng.integers(lo, hi, (batch,) + tuple(in_shape[1:]), dtype=dt)
    x[:5] = P.images(rng, in_shape, in_q, dt, 5, rows=True)
    xd = torch.as_tensor(x).cuda()
    n = batch * m.output_elems
    got = {}
    for fusion in (True, False):
        buf, out = _guarded(n, xd.dtype)
        m.set_fusion(fusion)
        try:
            if not ROUTING_SWITCHED:
                assert (names(m)[1] == FUSED) == fusion, names(m)
            m.run_quantized(xd, out=out)
            m.sync()
        finally:
            m.set_fusion(True)
        assert _intact(buf, n), ("a guard byte was written", "one launch" if fusion else "two launches")
        got[fusion] = out.cpu().numpy().reshape(batch, -1)
    diff = np.flatnonzero((got[True] != got[False]).any(axis=1))
    assert diff.size == 0, ("images that differ between one launch and two", diff[:8].tolist(), int(diff.size), "steps", sorted(set((diff // G).tolist()))[:8])
    idx = sorted({0, 1, G - 1, G, 2 * G - 1, batch // 2, batch - r - 1, batch - r, batch - 1})
    want = pad_ref.segments(tw, O, in_shape, in_q, layers, elem)(x[idx].reshape(len(idx), -1))[-1]
    bad = [i for k, i in enumerate(idx) if not np.array_equal(got[True][i], want[k])]
    assert not bad, ("images that differ from the reference", bad)
