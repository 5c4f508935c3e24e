"""The chain kernel (k_chain.hip chain_rt) under every plan autotune can install, not only the one the cost model picks.

How chain_rt runs is a host-made plan (k_chain.hip chain_plan: images per step G, double buffering of pair 0's input tile, the cut
of a run of pairs into launches, and from those the LDS layout, the unit ranges per wave, the 8- or 16-wave instance ...).  The
public mf_model_set_autotune times and installs plans the cost model never produces (G = 3 * 2^k, both dbuf values, measured cuts).
MF_DEV=1 MF_CHAIN_PLAN="len:G:dbuf,..." (csrc/mf_switches.hpp) forces a plan through the same functions and feasibility checks,
deterministically, and fails the preparation if it cannot be realised -- so "this plan ran" is a fact, not a hope.

The sweep: one child process per model (this file run as a script), MF_* stripped from its environment; the switch is re-read at
every preparation, so one child walks all plans of its model.  Per plan: the labels show the forced cut and G, the forced line of
MF_CHAIN_VERBOSE shows dbuf / nwave / LDS bytes; every image of ragged batches is bit-equal to the oracle and to the layer-wise
kernels; the output lands in the middle of a 0x5A-filled buffer whose other bytes stay; a second launch gives the same bytes.

Batches: 5 G + 3 for every plan (ragged, several steps, one step per workgroup), and 1025 G + 3 for the smallest G of a model (the
three smallest where that stays a few thousand images): a chain launch has at most 512 workgroups, so only there does a workgroup
walk SEVERAL steps -- what the double buffer, stage_after and the step queue are about.  (Larger G at that many steps would cost
the oracle minutes.)
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu

G_LIST = [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128]
CUTS4 = [[4], [2, 2], [1, 3], [3, 1], [1, 2, 1], [1, 1, 1, 1], [2, 0, 1]]   # (0: that pair as its two separate operators)
FOUR = [("dw", 0, 3, 1), ("conv", 32, 1, 1), ("dw", 0, 3, 1), ("conv", 32, 1, 1), ("dw", 0, 3, 2), ("conv", 64, 1, 1), ("dw", 0, 3, 1), ("conv", 64, 1, 1)]
# name -> input shape, operators, element type, weights within +-wmax of the middle (None: full range), max_cg (the images one
# depthwise unit spans: 16 / (CX CY), the largest over the pairs; G is a multiple of it -- chain_plan), the epilogue mode expected
MODELS = {
    # CX = 8, CY = 2, CG = 1: every G from 1 up; the row pitch pad search (CY > 1); one channel group: the RES instance
    "8x8x16": dict(shape=(8, 8, 16), convs=[("dw", 0, 3, 1), ("conv", 16, 1, 1)], elem=tw.INT8, max_cg=1),
    # odd sizes: CX = CY = 1, CG = 16; P = 25 G leaves a ragged 16-pixel chunk at G = 16 * odd.
    # chain_plan: G % max_cg == 0, so this model has no G below 16 and none that is not a multiple of 16 (3 * 2^k * 16 = 48, 96 exist)
    "5x5x32": dict(shape=(5, 5, 32), convs=[("dw", 0, 3, 1), ("conv", 32, 1, 1)], elem=tw.INT8, max_cg=16),
    # stride 2 into an odd size; the image pitch pad (CG > 1).  The same G rule as above
    # chain_plan's LDS budget (150 KB) on top of it: 16 halo'd 12x12x32 tiles are 74 KB, 87 KB with the rest of the plan, so G = 16 is
    # this model's ONLY plan: no G = 3 * 16 (no_g3), and the tile does not fit twice (no_dbuf1).  The parent checks that both were
    # tried and refused; 6x6x32s2 below is the same rule set at a size where they exist
    "10x10x32s2": dict(shape=(10, 10, 32), convs=[("dw", 0, 3, 2), ("conv", 64, 1, 1)], elem=tw.INT8, max_cg=16, no_g3=True, no_dbuf1=True),
    "6x6x32s2": dict(shape=(6, 6, 32), convs=[("dw", 0, 3, 2), ("conv", 64, 1, 1)], elem=tw.INT8, max_cg=16),
    # N = 48 is three 16-channel output tiles: chain_plan cuts N / 16 into a power-of-two number of blocks of at most chain_tbm() = 2
    # tiles (MF_CHAIN_TBM1 = 2; TB = 3 needs 4), so this pair has NO chain plan and runs as its two operators (no_chain): every
    # forced plan must be refused -- also by a model that has no run of pairs at all -- and the operators still match the oracle
    "12x12x48-u8": dict(shape=(12, 12, 48), convs=[("dw", 0, 3, 1), ("conv", 48, 1, 1)], elem=tw.UINT8, max_cg=1, no_chain=True),
    # ... so NQ = 3 (no swizzle, lgNQ = -1) and the u8 (XR4) instance are pinned with N = 64; 8 waves up to G = 4, 16 from dbuf at G = 4
    "12x12x48-64-u8": dict(shape=(12, 12, 48), convs=[("dw", 0, 3, 1), ("conv", 64, 1, 1)], elem=tw.UINT8, max_cg=1),
    # KSC = 4, full-range weights: 256-deep accumulators leave (-2^22, 2^22), epilogue mode 0 (v_cvt); one workgroup per CU
    "4x4x256": dict(shape=(4, 4, 256), convs=[("dw", 0, 3, 1), ("conv", 256, 1, 1)], elem=tw.INT8, max_cg=1, mode=0),
    # C < 16: two pixels form one 16-channel superpixel; such a pair only ever runs alone
    "16x16x8": dict(shape=(16, 16, 8), convs=[("dw", 0, 3, 1), ("conv", 16, 1, 1)], elem=tw.INT8, max_cg=1),
    "16x16x8s2": dict(shape=(16, 16, 8), convs=[("dw", 0, 3, 2), ("conv", 16, 1, 1)], elem=tw.INT8, max_cg=1),
    # four pairs 8x8x32 -> 32 -> 32 (s2) -> 4x4x64 -> 64: every cut; pairs 0 and 1 have one geometry and (in_zp = the type's minimum,
    # like every later tensor) one zero point, so they share a tile region -- unless pair 0's is double buffered; stage_after > 0; otab
    "four": dict(shape=(8, 8, 32), convs=FOUR, elem=tw.INT8, max_cg=1, in_zp=-128, cuts=CUTS4),
    # ... as u8 with small weights: the bit-pattern epilogues (modes 1 / 2) inside a chain
    "four-u8-small": dict(shape=(8, 8, 32), convs=FOUR, elem=tw.UINT8, max_cg=1, in_zp=0, wmax=40, cuts=CUTS4),
}
PAD = 4096          # guard bytes on either side of the output (a multiple of the widest store's alignment)
MULTI_STEPS = 1025  # steps of the long batches: more than the 512 workgroups of a chain launch, so that workgroups walk several steps


def blob_of(name):
    s = MODELS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    return tw.conv_net(rng, s["shape"], s["convs"], s["elem"], wmax=s.get("wmax"), in_zp=s.get("in_zp"), act_scale=6.0 / 255.0)


def plan_text(cut, G, dbuf):
    """one entry per segment; a single pair's dbuf is forced only in a one-pair model (in a cut it follows the planner's rule)"""
    return ",".join("0:0:-1" if n == 0 else "%d:%d:%d" % (n, G, dbuf if n == 1 else -1) for n in cut)


# ------------------------------------------------------------------------------------------------------------------------------
# the child: python tests/test_gpu_chain_plans.py sweep MODEL
# ------------------------------------------------------------------------------------------------------------------------------
class Stderr:
    """what the library writes to file descriptor 2 while the block runs (the MF_CHAIN_VERBOSE lines of one preparation)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        if exc[0] is not None:
            sys.stderr.write(self.text)
        return False


FORCED = re.compile(r"chain plan forced: pairs (\d+)\.\.(\d+) G (\d+) dbuf (\d+) nwave (\d+) lds (\d+)")
CREATED = re.compile(r"\] (chain_rt<\S+>) est \S+ us/image/CU lds (\d+) nwave (\d+) dbuf (\d+)")


def segments_of(m):
    """[(first pair, pairs, label or None)] from the kernel labels of a prepared model of depthwise + 1x1 pairs only"""
    segs, i = [], 0
    while i < m.num_ops:
        k = m.op(i)["kernel"]
        if k.startswith("chain_rt<"):
            n = k.count("|") + 1
            for j in range(i + 1, i + 2 * n):
                assert m.op(j)["kernel"].startswith("(fused"), (j, m.op(j)["kernel"])
            segs.append((i // 2, n, k))
            i += 2 * n
        else:
            assert not k.startswith("(fused") and not m.op(i + 1)["kernel"].startswith("(fused"), (i, k)
            segs.append((i // 2, 0, None))
            i += 2
    return segs


def child_sweep(name):
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    from oracle import oracle as O
    O.build()
    spec = MODELS[name]
    blob = blob_of(name)
    mc, cuts = spec["max_cg"], spec.get("cuts", [[1]])
    single = cuts == [[1]]
    # the long batches (several steps per workgroup): the three smallest G; only the smallest where that is already thousands of
    # images (max_cg = 16) or a 256-deep product per pixel -- the oracle's time
    multi_G = [g for g in G_LIST if g % mc == 0][:3 if mc == 1 and spec["shape"][2] < 256 else 1]
    om = O.Model(blob)
    m0 = mf.Model(blob)
    lo, hi = (0, 256) if m0.dtype == np.uint8 else (-128, 128)
    nmax = max(5 * 128 + 3, MULTI_STEPS * max(multi_G) + 3)
    xq = np.random.default_rng(len(name)).integers(lo, hi, (nmax, m0.input_elems)).astype(m0.dtype)
    xq[0], xq[1] = hi - 1, lo
    want = om.run_quantized_batch(xq).reshape(nmax, -1)      # the oracle, once, for the longest batch; a plan's batch is a prefix
    assert len(np.unique(want)) > 200, "the model's outputs do not spread"
    x_dev = torch.from_numpy(xq).cuda()
    tdt = torch.uint8 if m0.dtype == np.uint8 else torch.int8
    npairs = m0.num_ops // 2
    del m0

    def check(m, batch, tag):
        """(b) oracle and layer-wise parity on every image, (c) the guard bytes, (d) a second launch"""
        x = x_dev[:batch].reshape((batch,) + m.input_shape)
        n = batch * m.output_elems
        big = torch.full((PAD + n + PAD,), 0x5A, dtype=tdt, device="cuda")
        got = m.run_quantized(x, out=big[PAD:PAD + n]).reshape(batch, -1).cpu().numpy()
        whole = big.cpu().numpy()
        assert (whole[:PAD] == 0x5A).all() and (whole[PAD + n:] == 0x5A).all(), (tag, batch, "bytes outside the output were written")
        bad = np.argwhere(got != want[:batch])
        assert bad.size == 0, (tag, batch, "differs from the oracle", len(bad), bad[:4].tolist(), sorted({int(b[0]) for b in bad})[:12])
        again = m.run_quantized(x).reshape(batch, -1).cpu().numpy()
        assert np.array_equal(again, got), (tag, batch, "second launch differs")
        m.set_fusion(False)
        lw = m.run_quantized(x).reshape(batch, -1).cpu().numpy()
        m.set_fusion(True)
        assert np.array_equal(lw, got), (tag, batch, "differs from the layer-wise kernels")
        return got

    def batches(G, full):
        b = [5 * G + 3] + ([MULTI_STEPS * G + 3] if G in multi_G else [])
        return sorted(set(([1, G - 1, G, G + 1] if full else []) + b) - {0})

    # ---- the planner's own plan ----
    os.environ.pop("MF_CHAIN_PLAN", None)
    with Stderr() as err:
        m = mf.Model(blob)
        m.prepare(1)
    created = {k: (int(l), int(w), int(d)) for k, l, w, d in CREATED.findall(err.text)}   # (the last line of a name is the installed plan)
    own = segments_of(m)
    own_plan, own_out = [], None
    for first, n, label in own:
        if n == 0:
            own_plan.append("0:0:-1")
            print("PLAN planner pair=%d unfused" % first)
            continue
        G = int(label[label.rindex(";G") + 2:-1])
        lds, nwave, dbuf = created[label]
        own_plan.append("%d:%d:%d" % (n, G, dbuf if n == 1 else -1))
        print("PLAN planner pairs=%d..%d G=%d dbuf=%d nwave=%d lds=%d mode=%d label=%s" % (first, first + n - 1, G, dbuf, nwave, lds, m.op_epilogue_mode(2 * first), label))
    own_G = max([int(s.split(":")[1]) for s in own_plan] + [mc])
    own_out = check(m, 5 * own_G + 3, "planner")
    own_plan = ",".join(own_plan)
    del m

    # ---- the sweep ----
    plans = [(cut, G, d) for cut in cuts for G in G_LIST for d in ((0, 1) if single else (-1,))]
    full_done, replayed = False, False
    for text in [plan_text(*p) for p in plans] + [own_plan]:
        replay = text == own_plan
        if replay and replayed:
            continue
        os.environ["MF_CHAIN_PLAN"] = text
        m = mf.Model(blob)
        try:
            with Stderr() as err:
                m.prepare(1)
        except _lib.MicroflowError as e:
            assert e.status == _lib.MF_ERR_UNSUPPORTED and "MF_CHAIN_PLAN segment" in e.message, (text, e)   # any other status is a failure
            print("PLAN forced plan=%s infeasible (%s)" % (text, e.message.split(": ")[-1]))
            assert not replay or spec.get("no_chain"), "the planner's own plan cannot be forced"
            continue
        forced = {int(a): (int(b), int(g), int(d), int(w), int(l)) for a, b, g, d, w, l in FORCED.findall(err.text)}
        segs, asked, at = segments_of(m), text.split(","), 0
        assert len(segs) == len(asked), (text, segs)
        Gs = []
        for (first, n, label), entry in zip(segs, asked):       # (a) the labels show the forced cut and G, the forced line dbuf
            ln, G, d = map(int, entry.split(":"))
            assert first == at and n == ln, (text, segs)
            at += max(ln, 1)
            if ln == 0:
                print("PLAN forced plan=%s pair=%d unfused" % (text, first))
                continue
            last, fG, fd, nwave, lds = forced[first]
            assert last == first + n - 1 and label.endswith(";G%d>" % fG) and (G == 0 or fG == G) and (d < 0 or fd == d), (text, label, forced[first])
            mode = m.op_epilogue_mode(2 * first)
            assert mode == spec.get("mode", mode) and (mode >= 1 or "mode" in spec), (text, mode)
            assert nwave in (8, 16) and lds <= 150 * 1024
            Gs.append(fG)
            print("PLAN forced plan=%s pairs=%d..%d G=%d dbuf=%d nwave=%d lds=%d mode=%d ran label=%s" % (text, first, last, fG, fd, nwave, lds, mode, label))
        assert at == npairs
        G = max(Gs + [mc])
        # the whole batch sweep on one plan per model: the first with an odd number of image groups (where the model has none: its smallest G)
        full = not full_done and G == (mc if spec.get("no_g3") else 3 * mc)
        full_done = full_done or full
        for b in batches(G, full):
            got = check(m, b, text)
            if replay and b == 5 * own_G + 3:
                assert np.array_equal(got, own_out), "the planner's plan, forced, gives other bytes"
        if replay:
            replayed = True
            print("PLAN replay plan=%s reproduces the planner's" % text)
        del m
    if spec.get("no_chain"):
        assert own == [(0, 0, None)] and not replayed and not full_done
    else:
        assert replayed and full_done
    print("DONE %s" % name)


# ------------------------------------------------------------------------------------------------------------------------------
# the parent
# ------------------------------------------------------------------------------------------------------------------------------
def run_child(args, extra=None):
    """children run one after another, with no MF_* variable of the caller's (a run under scripts/switch_matrix.sh tests the same thing)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env.update(MF_DEV="1", MF_CHAIN_VERBOSE="1")
    env.update(extra or {})
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    table = "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith(("PLAN", "DONE", "LABELS")))
    assert r.returncode == 0, "%s\n%s" % (table[-6000:], r.stderr[-4000:])
    return table


RAN = re.compile(r"PLAN forced plan=(\S+) pairs=(\d+)\.\.(\d+) G=(\d+) dbuf=(\d+) nwave=(\d+) lds=(\d+) mode=(\d+) ran")


@pytest.mark.parametrize("name", list(MODELS))
def test_every_plan_of_the_sweep_is_bit_exact(name):
    spec = MODELS[name]
    table = run_child(["sweep", name])
    print(table)
    assert ("DONE " + name) in table, table
    mc, cuts = spec["max_cg"], spec.get("cuts", [[1]])
    feasible_G = [g for g in G_LIST if g % mc == 0]
    ran = [(p, int(a), int(b), int(g), int(d)) for p, a, b, g, d, _, _, _ in RAN.findall(table)]
    if spec.get("no_chain"):
        assert not ran and table.count(" infeasible (") >= len(G_LIST) * 2 and "PLAN planner pair=0 unfused" in table, table
        return
    # whole-model plans of the sweep proper (one G in every segment), by cut
    by_cut = {}
    for cut in cuts:
        for G in G_LIST:
            for d in ((0, 1) if cuts == [[1]] else (-1,)):
                text = plan_text(cut, G, d)
                rows = [r for r in ran if r[0] == text]
                if rows:
                    assert len(rows) == sum(1 for n in cut if n > 0) and all(r[3] == G for r in rows), (text, rows)
                    by_cut.setdefault(tuple(cut), []).append((G, [r[4] for r in rows]))
    # the conditions that keep the sweep from hiding a failure: every cut ran, and in every cut the smallest feasible G (= max_cg),
    # a G = 3 * 2^k * max_cg, and the largest G any cut of the model ran (the LDS budget is the only other limit, and it is the
    # cut's business: the longest chain holds the most tiles)
    for cut in cuts:
        Gs = sorted({g for g, _ in by_cut.get(tuple(cut), [])})
        assert Gs, (cut, "never ran", table)
        assert Gs[0] == feasible_G[0] == mc, (cut, Gs)
        if spec.get("no_g3"):
            assert Gs == [mc] and ("plan=%s infeasible" % plan_text(cut, 3 * mc, 0)) in table, (cut, Gs)
        else:
            assert any(g % (3 * mc) == 0 and (g // (3 * mc)) & (g // (3 * mc) - 1) == 0 for g in Gs), (cut, Gs)
        assert set(Gs) <= set(feasible_G), (cut, Gs)
        # feasibility is monotonic in G (only the LDS budget grows with it): what ran is a prefix of the feasible list
        assert Gs == feasible_G[:len(Gs)], (cut, Gs, feasible_G)
    if cuts == [[1]]:
        dbufs = {d for _, ds in by_cut[(1,)] for d in ds}
        # KSC = 4 included: at G = 1 the 4x4x256 tile fits twice
        if spec.get("no_dbuf1"):
            assert dbufs == {0} and ("plan=%s infeasible" % plan_text([1], mc, 1)) in table, (name, dbufs)
        else:
            assert dbufs == {0, 1}, (name, dbufs)
    else:
        assert any(1 in ds for cut, rows in by_cut.items() if cut[0] >= 2 for _, ds in rows), "no chain ran double buffered"
    assert "reproduces the planner's" in table


# ---- the public autotune entry --------------------------------------------------------------------------------------------------
def labels_of(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def autotuned_parity(mf, O, blob, batch, seed):
    import torch
    om = O.Model(blob)
    probe = mf.Model(blob)
    lo, hi = (0, 256) if probe.dtype == np.uint8 else (-128, 128)
    xq = np.random.default_rng(seed).integers(lo, hi, (batch, probe.input_elems)).astype(probe.dtype)
    xq[0], xq[1] = hi - 1, lo
    want = om.run_quantized_batch(xq).reshape(batch, -1)
    x = torch.from_numpy(xq).cuda().reshape((batch,) + probe.input_shape)
    for attempt in range(2):     # the two measured plans may differ; both must be exact
        m = mf.Model(blob, autotune=True)
        m.prepare(batch)
        labels = labels_of(m)
        print("autotune attempt %d:" % attempt, [k for k in labels if k and not k.startswith("(fused")])
        got = m.run_quantized(x).reshape(batch, -1).cpu().numpy()
        assert np.array_equal(got, want), (labels, np.argwhere(got != want)[:4].tolist())
        m.set_fusion(False)
        lw = m.run_quantized(x).reshape(batch, -1).cpu().numpy()
        assert np.array_equal(lw, got), labels


def test_autotuned_four_pair_model_is_bit_exact(O):
    import microflow_rs_amd as mf
    autotuned_parity(mf, O, blob_of("four"), 5 * 48 + 3, 5)


def test_autotuned_generated_model_is_bit_exact(O):
    import microflow_rs_amd as mf
    autotuned_parity(mf, O, tw.person_detect_like(np.random.default_rng(164), 64, 1.0), 131, 6)


def test_set_autotune_after_prepare_is_refused():
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    m = mf.Model(blob_of("four"))
    m.set_autotune(True)
    m.set_autotune(False)
    m.prepare(4)
    with pytest.raises(_lib.MicroflowError) as e:
        m.set_autotune(True)
    assert e.value.status == _lib.MF_ERR_INVALID_ARG


def test_table_shapes_are_not_affected_by_autotune():
    import microflow_rs_amd as mf
    from tests.conftest import model_path
    a, b = mf.Model(model_path("person_detect"), autotune=True), mf.Model(model_path("person_detect"))
    a.prepare(8), b.prepare(8)
    assert labels_of(a) == labels_of(b)


def child_labels(name):
    """LABELS lines: the model autotuned; not autotuned; and, the autotuned cut forced with the planner's G and double buffering"""
    import microflow_rs_amd as mf
    blob = blob_of(name)
    a = mf.Model(blob, autotune=True)
    a.prepare(4)
    print("LABELS autotuned %r" % labels_of(a))
    b = mf.Model(blob)
    b.prepare(4)
    print("LABELS planned %r" % labels_of(b))
    os.environ["MF_CHAIN_PLAN"] = ",".join("0:0:-1" if n == 0 else "%d:0:-1" % n for _, n, _ in segments_of(a))
    c = mf.Model(blob)
    c.prepare(4)
    print("LABELS replanned %r" % labels_of(c))


def labels_from(table):
    return {ln.split()[1]: ln.split(" ", 2)[2] for ln in table.splitlines() if ln.startswith("LABELS")}


def test_environment_overrides_the_handles_autotune_flag():
    """MF_DEV=1 MF_CHAIN_AUTOTUNE=0: the labels of an autotune=True model are the planner's"""
    got = labels_from(run_child(["labels", "four"], {"MF_CHAIN_AUTOTUNE": "0"}))
    assert got["autotuned"] == got["planned"] and "chain_rt<" in got["planned"], got


def test_tune_g_off_keeps_the_planners_images_per_step():
    """MF_DEV=1 MF_CHAIN_TUNE_G=0: autotune still chooses the cut by measurement, but every label carries the G the planner gives that cut"""
    got = labels_from(run_child(["labels", "four"], {"MF_CHAIN_TUNE_G": "0"}))
    assert got["autotuned"] == got["replanned"] and "chain_rt<" in got["autotuned"], got


if __name__ == "__main__":
    {"sweep": child_sweep, "labels": child_labels}[sys.argv[1]](sys.argv[2])
