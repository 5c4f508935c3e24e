"""Sliding windows on the device (include/microflow_amd.h section 5; k_windows.hip), every comparison bit for bit:
the gather alone against numpy over window rows of 1 .. 257 elements, hops that are and are not whole dwords, sources at byte
offsets 0 .. 3, padded rows, several sources, first != 0, destinations at every alignment with guard bytes; the quantising
gather against mf_quantize[_u8] on the materialised windows at half-way points, NaN, infinities, saturation and denormals, with
and without the fast division; speech, its u8 twin, person_detect, a 3-channel convolution net and sine over windows against
run_quantized / predict / predict_quantized on the materialised windows and against the CPU oracle; chunking and its launch
counts; graph mode left alone; guards around the outputs and the source unchanged."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, model_path

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

GUARD = 0x5A


def _np_dt(u8):
    return np.uint8 if u8 else np.int8


# ---- 1. the gather alone ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """random bytes, on the host and on the device, that every gather case slices its source from"""
    import torch
    a = np.random.default_rng(1).integers(-128, 128, 1 << 16).astype(np.int8)
    return a, torch.as_tensor(a).cuda()


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("we", [1, 3, 13, 16, 40, 96, 257])
def test_gather_against_numpy(pool, we, u8):
    import microflow_rs_amd as mf
    import torch
    host, dev = pool
    if u8:
        host, dev = host.view(np.uint8), dev.view(torch.uint8)
    case = 0
    for wr in (1, 5):
        for he in (1, 3, 4, 16):
            for hr in (1, 2):
                for pad in (0, 1, 7):
                    for ns in (1, 3):
                        # the source is win + 3 hops each way: 4 x 4 windows per source, no combination left out
                        sr, se = wr + 3 * hr, we + 3 * he
                        pitch = se + pad
                        one = (sr - 1) * pitch + se
                        w = mf.Windows(src_rows=sr, src_row_elems=se, win_rows=wr, win_row_elems=we, hop_rows=hr, hop_elems=he,
                                       src_pitch=pitch, n_sources=ns, src_stride=one + 5 if ns > 1 else None)
                        total = 16 * ns
                        assert w.total == total
                        base = case % 4                         # source base pointer at byte offsets 0 .. 3 (a sliced tensor)
                        start = 64 * (case % 7) + base
                        first, count = ((0, total) if case % 3 else (3, total - 5))
                        E = wr * we
                        want = w.materialize(host[start: start + w.source_elems])[first: first + count]
                        g0 = 16 + case % 16                     # the destination at every 16-byte phase, guards on both sides
                        buf = torch.full((g0 + count * E + 32,), GUARD, dtype=dev.dtype, device="cuda")
                        out = buf[g0: g0 + count * E]
                        got = mf.gather_windows(dev[start: start + w.source_elems], w, first, count, out=out)
                        assert got.data_ptr() == out.data_ptr()
                        b = buf.cpu().numpy()
                        what = (we, wr, he, hr, pad, ns, base, first, count, g0)
                        assert np.array_equal(b[g0: g0 + count * E].reshape(count, E), want), what
                        assert (b[:g0].view(np.uint8) == GUARD).all() and (b[g0 + count * E:].view(np.uint8) == GUARD).all(), what
                        case += 1
    assert case == 2 * 4 * 2 * 3 * 2


def test_gather_window_size_not_a_multiple_of_16_many_blocks(pool):
    """enough output for several workgroups, windows of 13 x 5 = 65 bytes: chunks that straddle rows AND windows"""
    import microflow_rs_amd as mf
    host, dev = pool
    w = mf.Windows(src_rows=120, src_row_elems=300, win_rows=5, win_row_elems=13, hop_rows=1, hop_elems=1, src_pitch=301)
    assert w.total == 116 * 288
    want = w.materialize(host[1: 1 + w.source_elems])
    got = mf.gather_windows(dev[1: 1 + w.source_elems], w).cpu().numpy()
    assert np.array_equal(got, want)


# ---- 2. gather + quantise -----------------------------------------------------------------------------------------------------
def _f32_source(n, scale, zp, u8, seed):
    """random representable values with the hard ones planted: ties in both signs, +-0, denormals, far beyond saturation, +-inf, NaN"""
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if u8 else (-128, 128)
    sc = np.float32(scale)
    with np.errstate(all="ignore"):
        x = ((rng.integers(lo - 3, hi + 3, n) - zp).astype(np.float32) * sc).astype(np.float32)
        ks = np.array([lo - 1, lo, lo + 1, zp - 1, zp, hi - 2, hi - 1] + list(rng.integers(lo, hi, 9)), np.float64)
        half = ((ks + 0.5 - zp).astype(np.float32) * sc).astype(np.float32)
        special = np.concatenate([half, -half, np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1e30, -1e30, 3.4e38, -3.4e38,
                                                         np.float32(hi + 1000 - zp) * sc, np.float32(lo - 1000 - zp) * sc, np.inf, -np.inf, np.nan,
                                                         -np.nan], np.float32)]).astype(np.float32)
        # a quarter of the source is random bit patterns: every exponent, NaNs and denormals among them
        k = n // 4
        x[rng.choice(n, k, replace=False)] = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32).view(np.float32)
        for rep in range(max(1, n // (4 * special.size))):
            k = min(n, special.size)
            x[rng.choice(n, k, replace=False)] = special[rng.permutation(special.size)[:k]]
    return x


def _quantize_dense(x_dev, scale, zp, u8):
    import torch
    from microflow_rs_amd import _lib
    out = torch.empty(x_dev.numel(), dtype=torch.uint8 if u8 else torch.int8, device="cuda")
    fn = _lib.lib().mf_quantize_u8 if u8 else _lib.lib().mf_quantize
    _lib.check(fn(0, x_dev.data_ptr(), x_dev.numel(), float(scale), int(zp), out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


QUANT_GEOMS = [dict(src_rows=9, src_row_elems=61, win_rows=3, win_row_elems=40, hop_rows=2, hop_elems=3, src_pitch=64, n_sources=2, src_stride=700),
               dict(src_rows=60, src_row_elems=40, win_rows=49, win_row_elems=40, hop_rows=1, hop_elems=1),
               dict(src_rows=7, src_row_elems=30, win_rows=5, win_row_elems=13, hop_rows=1, hop_elems=1)]


def _check_gather_quantize(scale, zp, u8):
    import microflow_rs_amd as mf
    import torch
    for gi, geom in enumerate(QUANT_GEOMS):
        w = mf.Windows(**geom)
        x = _f32_source(w.source_elems, scale, zp, u8, 50 + gi)
        xd = torch.as_tensor(x).cuda()
        total = w.total
        first, count = (2, total - 3) if gi == 0 else (0, total)
        dense = torch.as_tensor(w.materialize(x)[first: first + count].copy()).cuda()
        want = _quantize_dense(dense, scale, zp, u8)
        E = w.window_elems
        buf = torch.full((5 + count * E + 32,), GUARD, dtype=torch.uint8 if u8 else torch.int8, device="cuda")
        mf.gather_windows(xd, w, first, count, quantize=(scale, zp, _np_dt(u8)), out=buf[5: 5 + count * E])
        b = buf.cpu().numpy()
        diff = np.flatnonzero(b[5: 5 + count * E] != want)
        assert diff.size == 0, (scale, zp, u8, geom, diff[:5], b[5:][diff[:5]], want[diff[:5]])
        assert (b[:5].view(np.uint8) == GUARD).all() and (b[5 + count * E:].view(np.uint8) == GUARD).all()


def _model_quant(name):
    import microflow_rs_amd as mf
    m = mf.Model(model_path(name))
    return float(m.input_scale), int(m.input_zero_point)


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("name", ["speech", "person_detect"])
def test_gather_quantize_equals_quantize_on_materialised_windows(name, u8):
    scale, zp = _model_quant(name)
    _check_gather_quantize(scale, zp + (128 if u8 else 0), u8)


def _unverified_pair():
    """a (scale, zero point) whose fast division the device check rejects, or None"""
    from microflow_rs_amd import _lib
    for scale in (3.0e38, 2.0e38, 1.5e-38, 3.3e38, 1.0e38, 7.0e-39):
        s = np.float32(scale)
        bad = C.c_uint64(0)
        with np.errstate(all="ignore"):
            rcp = np.float32(1.0 / np.float64(s))
        _lib.check(_lib.lib().mf_verify_quant_div(0, float(s), float(rcp), 3, 0, C.byref(bad)))
        if bad.value:
            return float(s), 3
    return None


def test_gather_quantize_where_the_fast_division_is_not_verified():
    pair = _unverified_pair()
    if pair is not None:
        _check_gather_quantize(pair[0], pair[1], False)
        return
    # no trial scale is rejected on this device: take the fast division away by the developer switch, in a process of its own
    code = ("import sys; sys.path.insert(0, %r); import tests.test_gpu_windows as t; t._check_gather_quantize(%r, %r, False); print('WINDOWS-OK')"
            % (ROOT, *_model_quant("speech")))
    env = dict(os.environ, MF_DEV="1", MF_NO_FAST_QUANT_DIV="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "WINDOWS-OK" in out.stdout, out.stdout + out.stderr


# ---- 3. models ------------------------------------------------------------------------------------------------------------------
def _blob(name):
    import tflite_writer as tw
    if name == "speech-u8":
        from make_u8_model import to_u8
        return bytes(to_u8(open(model_path("speech"), "rb").read()))
    if name == "conv3":
        return tw.conv_net(np.random.default_rng(77), (12, 12, 3), [("conv", 8, 3, 1), ("dw", 0, 3, 2), ("conv", 16, 1, 1)], head=5)
    return open(model_path(name), "rb").read()


def _windows(case):
    import microflow_rs_amd as mf
    return {
        "speech": lambda: mf.Windows.frames(64, 40, 49),                                             # 16 windows
        "speech-pitch43": lambda: mf.Windows(src_rows=64, src_row_elems=40, win_rows=49, win_row_elems=40, src_pitch=43),
        "speech-u8": lambda: mf.Windows.frames(64, 40, 49),
        "pd-16": lambda: mf.Windows.image((112, 128), (96, 96), 1, (8, 16), n=2),                    # 18 windows
        "pd-5": lambda: mf.Windows.image((112, 128), (96, 96), 1, (8, 5), n=2),                      # 42, unaligned starts
        "conv3": lambda: mf.Windows.image((20, 23), (12, 12), 3, 1),                                 # 108, 3-element hop
        "sine": lambda: mf.Windows(src_rows=1, src_row_elems=37, win_rows=1, win_row_elems=1),       # degenerates to a batch
    }[case]()


CASES = {"speech": ("speech", 16), "speech-pitch43": ("speech", 16), "speech-u8": ("speech-u8", 16), "pd-16": ("person_detect", 18),
         "pd-5": ("person_detect", 42), "conv3": ("conv3", 108), "sine": ("sine", 37)}
_models, _cases = {}, {}


def _model(name):
    if name not in _models:
        import microflow_rs_amd as mf
        blob = _blob(name)
        m = mf.Model(blob)
        m.prepare(1)
        _models[name] = (m, blob)
    return _models[name]


class WinCase:
    """one model over one window set: the sources, the materialised windows and the references, computed once"""

    def __init__(self, case):
        import torch
        mname, n = CASES[case]
        self.m, self.blob = _model(mname)
        self.w = _windows(case)
        assert self.w.total == n and self.w.window_elems == self.m.input_elems
        rng = np.random.default_rng(len(case) * 131 + n)
        u8 = self.m.dtype == np.uint8
        lo, hi = (0, 256) if u8 else (-128, 128)
        self.n = n
        self.src = rng.integers(lo, hi, self.w.source_elems + 3).astype(self.m.dtype)[3:]            # (a host source at an odd address)
        self.fsrc = _f32_source(self.w.source_elems, self.m.input_scale, self.m.input_zero_point, u8, n)
        self.src_d = torch.as_tensor(np.concatenate([self.src[:1], self.src])).cuda()[1:]           # device source at byte offset 1
        self.fsrc_d = torch.as_tensor(self.fsrc).cuda()
        self.dense = self.w.materialize(self.src)
        self.fdense = self.w.materialize(self.fsrc)
        dense_d, fdense_d = torch.as_tensor(self.dense).cuda(), torch.as_tensor(self.fdense).cuda()
        self.want_q = self.m.run_quantized(dense_d).cpu().numpy().reshape(n, -1)
        self.want_pq = self.m.predict_quantized(dense_d).cpu().numpy().reshape(n, -1)
        self.want_p = self.m.predict(fdense_d).cpu().numpy().reshape(n, -1)


def _case(name):
    if name not in _cases:
        _cases[name] = WinCase(name)
    return _cases[name]


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint8)


@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("case", list(CASES))
def test_model_over_windows(case, where):
    c = _case(case)
    src, fsrc = (c.src, c.fsrc) if where == "host" else (c.src_d, c.fsrc_d)

    def host(t, n=c.n):
        return (t if where == "host" else t.cpu().numpy()).reshape(n, -1)
    got = host(c.m.run_windows(src, c.w))
    assert got.dtype == c.m.dtype and np.array_equal(got, c.want_q), np.flatnonzero((got != c.want_q).any(1))
    got = host(c.m.predict_quantized_windows(src, c.w))
    assert np.array_equal(_bits(got), _bits(c.want_pq))
    got = host(c.m.predict_windows(fsrc, c.w))
    assert np.array_equal(_bits(got), _bits(c.want_p))
    # a part of the windows: first != 0, count cut short
    first, count = c.n // 3, c.n - c.n // 3 - 1
    got = host(c.m.run_windows(src, c.w, first, count), count)
    assert np.array_equal(got, c.want_q[first: first + count])


@pytest.mark.parametrize("case", list(CASES))
def test_model_over_windows_against_the_oracle(O, case):
    c = _case(case)
    om = O.Model(c.blob)
    picks = sorted({0, c.n - 1, c.n // 4, c.n // 2, 3 * c.n // 4})
    want = om.run_quantized_batch(c.dense[picks]).reshape(len(picks), -1)
    got = c.m.run_windows(c.src, c.w).reshape(c.n, -1)[picks]
    assert np.array_equal(got, want), (picks, got, want)


# ---- 4. chunking -----------------------------------------------------------------------------------------------------------------
def _delta(m, fn):
    import torch
    torch.cuda.synchronize()
    before = m.device_ops()
    r = fn()
    return m.device_ops() - before, r


@pytest.mark.parametrize("name", ["speech", "speech-u8"])
def test_chunks_of_five_over_23_windows(name):
    import microflow_rs_amd as mf
    import torch
    blob = _blob(name)
    m = mf.Model(blob)
    m.prepare(1)
    u8 = m.dtype == np.uint8
    w = mf.Windows.frames(71, 40, 49)
    assert w.total == 23
    rng = np.random.default_rng(23)
    src = rng.integers(*((0, 256) if u8 else (-128, 128)), w.source_elems).astype(m.dtype)
    fsrc = _f32_source(w.source_elems, m.input_scale, m.input_zero_point, u8, 24)
    src_d, fsrc_d = torch.as_tensor(src).cuda(), torch.as_tensor(fsrc).cuda()
    whole = m.run_windows(src, w).copy()
    whole_p = m.predict_windows(fsrc, w).copy()
    assert np.array_equal(whole.reshape(23, -1), m.run_quantized(w.materialize(src)).reshape(23, -1))
    dense_d = torch.as_tensor(w.materialize(src)).cuda()
    # what one chunk costs through the entry points that exist without windows: five resident inputs, aligned buffers
    d_rq, _ = _delta(m, lambda: m.run_quantized(dense_d[:5]))
    d_pq, _ = _delta(m, lambda: m.predict_quantized(dense_d[:5]))
    assert d_rq >= 1 and d_pq >= 1
    m.set_window_chunk(5)
    try:
        for s, fs in ((src, fsrc), (src_d, fsrc_d)):
            on_host = isinstance(s, np.ndarray)
            d, got = _delta(m, lambda: m.run_windows(s, w))
            got = got if on_host else got.cpu().numpy()
            assert np.array_equal(got, whole)
            if u8:      # the gather replaces the input's move into the internal domain: a chunk costs what run_quantized costs
                assert d == 5 * d_rq, (d, d_rq)
            elif on_host:
                assert d == 5 * (1 + d_rq), (d, d_rq)
            else:
                # device-resident: chunk c's results go straight to out + 20 c bytes where that is 16-byte aligned, as run_quantized
                # writes them -- elsewhere run_quantized itself adds a copy; per chunk the count is 1 + run_quantized's AT THAT slice
                out = torch.empty((23, m.output_elems), dtype=torch.int8, device="cuda")
                want = 0
                for c0 in range(0, 23, 5):
                    xin = dense_d[c0: c0 + 5].clone()   # (an aligned input, as the gathered chunk is)
                    dc, _ = _delta(m, lambda: m.run_quantized(xin, out=out[c0: c0 + 5]))
                    want += 1 + dc
                d2, got2 = _delta(m, lambda: m.run_windows(s, w, out=out))
                assert d2 == want and want >= 5 * (1 + d_rq), (d2, want, d_rq)
                assert np.array_equal(got2.cpu().numpy(), whole)
            d, got = _delta(m, lambda: m.predict_windows(fs, w))
            got = got if on_host else got.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(whole_p))
            assert d == 5 * (1 + d_pq) - (5 if u8 else 0), (d, d_pq)   # (u8: predict_quantized's own input pass is not run either)
    finally:
        m.set_window_chunk(0)


# ---- 5. graph mode -----------------------------------------------------------------------------------------------------------------
def test_windows_run_eagerly_and_leave_the_graph_alone():
    import microflow_rs_amd as mf
    import torch
    m = mf.Model(model_path("speech"))
    m.prepare(8)
    c = _case("speech")
    x = torch.as_tensor(c.dense[:8].copy()).cuda()
    o = torch.empty((8, m.output_elems), dtype=torch.int8, device="cuda")
    m.set_graph(True)
    m.run_quantized(x, out=o)                       # eager
    m.run_quantized(x, out=o)                       # captured and launched
    m.run_quantized(x, out=o)                       # replayed
    g = m.graph_launches
    assert g == 2
    ref = o.cpu().numpy().copy()
    assert np.array_equal(ref, c.want_q[:8])
    for _ in range(2):                              # (16 windows against activation buffers for 8: two chunks, no regrowth)
        got = m.run_windows(c.src_d, c.w)
        assert m.graph_launches == g
        assert np.array_equal(got.cpu().numpy().reshape(c.n, -1), c.want_q)
        assert np.array_equal(m.run_windows(c.src, c.w).reshape(c.n, -1), c.want_q) and m.graph_launches == g
    o.zero_()
    m.run_quantized(x, out=o)
    assert m.graph_launches == g + 1 and np.array_equal(o.cpu().numpy(), ref)


# ---- 6. guards --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["speech", "speech-u8", "pd-5"])
def test_output_guards_and_source_unchanged(case):
    import torch
    from microflow_rs_amd import _lib
    c = _case(case)
    m, n, N = c.m, c.n, c.m.output_elems
    src_before, fsrc_before = c.src_d.clone(), c.fsrc_d.clone()
    tdt = torch.uint8 if m.dtype == np.uint8 else torch.int8
    for g0 in (16, 3):
        big = torch.full((g0 + n * N + 19,), GUARD, dtype=tdt, device="cuda")
        m.run_windows(c.src_d, c.w, out=big[g0: g0 + n * N])
        b = big.cpu().numpy()
        assert np.array_equal(b[g0: g0 + n * N].reshape(n, N), c.want_q)
        assert (b[:g0].view(np.uint8) == GUARD).all() and (b[g0 + n * N:].view(np.uint8) == GUARD).all()
    pat = np.float32(-1234.5)
    bigf = torch.full((7 + n * N + 9,), float(pat), dtype=torch.float32, device="cuda")
    for fn, s, want in ((m.predict_windows, c.fsrc_d, c.want_p), (m.predict_quantized_windows, c.src_d, c.want_pq)):
        bigf.fill_(float(pat))
        fn(s, c.w, out=bigf[7: 7 + n * N])
        b = bigf.cpu().numpy()
        assert np.array_equal(_bits(b[7: 7 + n * N]), _bits(want))
        assert (b[:7] == pat).all() and (b[7 + n * N:] == pat).all()
    assert torch.equal(c.src_d, src_before) and torch.equal(_as_u32(c.fsrc_d), _as_u32(fsrc_before))
    # host buffers, through the C entry points: guards around `out`, the source bit-identical
    L = _lib.lib()
    src, fsrc = c.src.copy(), c.fsrc.copy()
    hb = np.full(5 + n * N + 11, GUARD, m.dtype)
    _lib.check(L.mf_model_run_windows(m._h, src.ctypes.data_as(C.c_void_p), C.byref(c.w.desc()), 0, n, C.c_void_p(hb.ctypes.data + 5), _lib.MF_MEM_HOST))
    assert np.array_equal(hb[5: 5 + n * N].reshape(n, N), c.want_q) and (hb[:5] == GUARD).all() and (hb[5 + n * N:] == GUARD).all()
    hf = np.full(3 + n * N + 6, pat, np.float32)
    _lib.check(L.mf_model_predict_windows(m._h, fsrc.ctypes.data_as(C.c_void_p), C.byref(c.w.desc()), 0, n, C.c_void_p(hf.ctypes.data + 12), _lib.MF_MEM_HOST))
    assert np.array_equal(_bits(hf[3: 3 + n * N]), _bits(c.want_p)) and (hf[:3] == pat).all() and (hf[3 + n * N:] == pat).all()
    assert np.array_equal(src, c.src) and np.array_equal(fsrc.view(np.uint32), c.fsrc.view(np.uint32))


def _as_u32(t):
    import torch
    return t.view(torch.int32)
