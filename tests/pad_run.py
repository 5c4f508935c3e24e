"""What the GPU tests of the PAD + convolution launch share (tests/test_gpu_pad_conv.py, tests/test_gpu_pad_conv_steps.py): a model
prepared once with its expected tensors (tests/pad_ref.py), and the check of those tensors under every way of running a model."""
import os
import sys

import numpy as np

from tests import composed as C
from tests import pad_cases as P
from tests import pad_ref
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

FUSED = C.FUSED
ELEMS = {"i8": (tw.INT8, np.int8), "u8": (tw.UINT8, np.uint8)}


class Prepared:
    """one model on the device: prepared once, the expected tensors computed once and left unchanged"""
    def __init__(self, O, model, elem, dt, seed=3, batch=5, rows=False):
        import microflow_rs_amd as mf
        self.in_shape, self.in_q, self.layers = model
        self.dt, self.n = dt, batch
        self.m = mf.Model(tw.build_model(self.in_shape, self.in_q, self.layers, elem))
        self.m.prepare(self.n)
        self.x = P.images(np.random.default_rng(seed), self.in_shape, self.in_q, dt, batch, rows)
        self.ref = pad_ref.segments(tw, O, self.in_shape, self.in_q, self.layers, elem)   # images [B, in_elems] -> every operator's tensor
        self.outs = self.ref(self.x.reshape(self.n, -1))
        for t in self.outs:
            t.setflags(write=False)
        self.want = self.outs[-1]


def names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def _run(m, x, n):
    return np.asarray(m.run_quantized(x)).reshape(n, -1)


def check_every_way(p):
    import torch
    m, n = p.m, p.n
    got = _run(m, p.x, n)
    assert np.array_equal(got, p.want), ("default", names(m), int((got != p.want).sum()), np.argwhere(got != p.want)[:4].tolist())
    assert len(p.outs) == m.num_ops
    for i in range(m.num_ops):
        got = np.asarray(m.run_until(p.x, i)).reshape(n, -1)
        assert np.array_equal(got, p.outs[i]), ("run_until", i, m.op(i)["name"], m.op(i)["kernel"], int((got != p.outs[i]).sum()))
    for switch in (m.set_fusion, m.set_generic):
        on = switch == m.set_generic
        switch(on)
        try:
            got = _run(m, p.x, n)
        finally:
            switch(not on)
        assert np.array_equal(got, p.want), ("fusion off" if not on else "generic", int((got != p.want).sum()))
    # graph replay: the same device buffers three times -- eager, captured, replayed
    xd = torch.as_tensor(p.x).cuda()
    out = torch.empty((n,) + tuple(m.output_shape[1:]) if len(m.output_shape) > 1 else (n,), dtype=xd.dtype, device="cuda")
    m.set_graph(True)
    try:
        before = m.graph_launches
        for _ in range(3):
            out.zero_()
            m.run_quantized(xd, out=out)
            m.sync()
            got = out.cpu().numpy().reshape(n, -1)
            assert np.array_equal(got, p.want), ("graph", int((got != p.want).sum()))
        assert m.graph_launches >= before + 2
    finally:
        m.set_graph(False)
