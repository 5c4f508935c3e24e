"""Model.time_device (mf_model_time_device, what bench.py measures with): the timed passes and the per-operator sweep behind them.
The sweep walks the model with the same launches a run takes, an event behind each: it has to hand back one finite duration per
operator, add nothing to device_ops() -- the timed passes alone count, one device-fed run each --, and leave the activation buffers
and the launch state as a predict_quantized expects them."""
import math

import numpy as np
import pytest

from tests.conftest import model_path

pytestmark = pytest.mark.gpu

BATCH, WARMUP, ITERS = 4, 1, 3


@pytest.mark.parametrize("name", ["sine", "speech", "person_detect"])
def test_time_device_with_and_without_the_sweep(name):
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd.synth import synth_i8
    m = mf.Model(model_path(name))
    m.prepare(BATCH)
    x = torch.from_numpy(synth_i8(5, 0, BATCH, m.input_elems)).cuda()
    d_out = torch.empty((BATCH, m.output_elems), dtype=torch.int8, device="cuda")
    want = m.predict_quantized(x).cpu().numpy().copy()  # (the first call also sizes the operators' scratch)
    before = m.device_ops()
    again = m.predict_quantized(x).cpu().numpy()
    one_run = m.device_ops() - before                    # what one device-fed predict_quantized of this batch adds
    assert one_run >= 1 and np.array_equal(again.view(np.uint32), want.view(np.uint32))

    added = {}
    for per_op in (True, False):
        before = m.device_ops()
        avg, per = m.time_device(x, d_out, BATCH, warmup=WARMUP, iters=ITERS, per_op=per_op)
        torch.cuda.synchronize()
        added[per_op] = m.device_ops() - before
        print("%s per_op=%s: avg %.4f ms, per-operator %s, device_ops +%d (one run: %d)" % (name, per_op, avg, per, added[per_op], one_run))
        assert math.isfinite(avg) and avg > 0
        if per_op:
            assert len(per) == m.num_ops
            assert all(math.isfinite(t) and t >= 0 for t in per), per
        else:
            assert per is None
    # the sweep's launches are not counted: with and without it, the timed passes alone
    assert added[True] == added[False] == (WARMUP + ITERS) * one_run, (added, one_run)
    # ... and it leaves the activation buffers and the launch state usable
    after = m.predict_quantized(x).cpu().numpy()
    assert np.array_equal(after.view(np.uint32), want.view(np.uint32))
