"""Sliding windows without a GPU (include/microflow_amd.h section 5): mf_windows_count and the index formula against
numpy.lib.stride_tricks.sliding_window_view over a few hundred random descriptions (several sources, pitch > row, hop > window);
every invalid description is MF_ERR_INVALID_ARG with a message naming the field, before any device is asked for; the new names are in
the header, the binding table and the Rust source at ABI version 3; a valid run_windows on a machine without a GPU is
MF_ERR_NO_DEVICE; and csrc/windows_spec.cpp, compiled alone with the host compiler under the address and undefined-behaviour
sanitizers (tests/cpp/windows_spec_main.cpp, a stand-alone program), gives the same answers on the same descriptions."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, model_path

FIELDS = ("n_sources", "src_stride", "src_rows", "src_row_elems", "src_pitch", "win_rows", "win_row_elems", "hop_rows", "hop_elems")
NEW_NAMES = ("mf_windows_count", "mf_window_gather", "mf_window_gather_quantize", "mf_window_gather_quantize_u8", "mf_model_run_windows",
             "mf_model_predict_windows", "mf_model_predict_quantized_windows", "mf_model_set_window_chunk")


def random_descriptions(n=300, seed=2024):
    """dicts of the nine fields; small enough to materialise"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        wr, we = int(rng.integers(1, 7)), int(rng.integers(1, 20))
        hr, he = int(rng.integers(1, 10)), int(rng.integers(1, 25))    # (hops beyond the window's own size among them)
        sr, se = wr + int(rng.integers(0, 12)), we + int(rng.integers(0, 30))
        pitch = se + int(rng.choice([0, 0, 1, 7, 13]))
        ns = int(rng.choice([1, 1, 2, 3, 5]))
        one = (sr - 1) * pitch + se
        stride = one + int(rng.choice([0, 1, 19])) if ns > 1 else int(rng.integers(0, 5))  # (ignored for one source, even when 0)
        out.append(dict(n_sources=ns, src_stride=stride, src_rows=sr, src_row_elems=se, src_pitch=pitch, win_rows=wr, win_row_elems=we,
                        hop_rows=hr, hop_elems=he))
    return out


def numpy_windows(d, src):
    """[total][win_rows * win_row_elems] by sliding_window_view, source by source"""
    from numpy.lib.stride_tricks import sliding_window_view
    res = []
    stride = d["src_stride"] if d["n_sources"] > 1 else 0
    for s in range(d["n_sources"]):
        one = src[s * stride: s * stride + (d["src_rows"] - 1) * d["src_pitch"] + d["src_row_elems"]]
        img = np.zeros((d["src_rows"], d["src_pitch"]), src.dtype)
        img.reshape(-1)[: one.size] = one
        v = sliding_window_view(img[:, : d["src_row_elems"]], (d["win_rows"], d["win_row_elems"]))[:: d["hop_rows"], :: d["hop_elems"]]
        res.append(v.reshape(-1, d["win_rows"] * d["win_row_elems"]))
    return np.concatenate(res)


def source_elems(d):
    return ((d["n_sources"] - 1) * d["src_stride"] if d["n_sources"] > 1 else 0) + (d["src_rows"] - 1) * d["src_pitch"] + d["src_row_elems"]


def invalid_descriptions():
    """(what, the word its message must hold, description, input_elems, first, count)"""
    ok = dict(n_sources=2, src_stride=500, src_rows=10, src_row_elems=40, src_pitch=44, win_rows=4, win_row_elems=8, hop_rows=2, hop_elems=3)
    E = 32

    def bad(what, word, first=0, count=1, input_elems=E, **kw):
        return (what, word, dict(ok, **kw), input_elems, first, count)
    total = 2 * 4 * 11
    return [bad("zero hop_rows", "hop_rows", hop_rows=0), bad("zero hop_elems", "hop_elems", hop_elems=0),
            bad("window taller than the source", "win_rows", win_rows=11, win_row_elems=8, input_elems=88),
            bad("window wider than the source", "win_row_elems", win_rows=1, win_row_elems=41, input_elems=41),
            bad("pitch shorter than a row", "src_pitch", src_pitch=39),
            bad("stride shorter than one source", "src_stride", src_stride=9 * 44 + 39),
            bad("window is not the model's input", "input_elems", input_elems=E + 1),
            bad("first + count beyond the total", "count", first=total - 3, count=4),
            bad("first beyond the total", "count", first=total + 1, count=0),
            bad("first + count wraps", "count", first=2 ** 64 - 1, count=2)]


def desc(d):
    from microflow_rs_amd import _lib
    return _lib.WindowsDesc(*[d[f] for f in FIELDS])


def test_count_and_index_formula_against_sliding_window_view():
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(7)
    seen = dict(multi=0, pitch=0, hop_gt=0)
    for d in random_descriptions():
        src = rng.integers(-128, 128, source_elems(d)).astype(np.int8)
        want = numpy_windows(d, src)
        per, total = C.c_size_t(), C.c_size_t()
        assert L.mf_windows_count(C.byref(desc(d)), C.byref(per), C.byref(total)) == _lib.MF_OK, d
        assert total.value == want.shape[0] and per.value * d["n_sources"] == total.value, d
        w = mf.Windows(**d)
        assert w.counts() == (per.value, total.value) and w.source_elems == source_elems(d)
        # the documented formula, element by element, is what materialize() evaluates with strides
        got = w.materialize(src)
        assert np.array_equal(got, want), d
        ny, nx = (d["src_rows"] - d["win_rows"]) // d["hop_rows"] + 1, (d["src_row_elems"] - d["win_row_elems"]) // d["hop_elems"] + 1
        for idx in {0, total.value - 1, int(rng.integers(0, total.value))}:
            s, iy, ix = idx // (ny * nx), idx // nx % ny, idx % nx
            r, e = int(rng.integers(0, d["win_rows"])), int(rng.integers(0, d["win_row_elems"]))
            at = (s * d["src_stride"] if d["n_sources"] > 1 else 0) + (iy * d["hop_rows"] + r) * d["src_pitch"] + ix * d["hop_elems"] + e
            assert src[at] == want[idx, r * d["win_row_elems"] + e], (d, idx, r, e)
        seen["multi"] += d["n_sources"] > 1
        seen["pitch"] += d["src_pitch"] > d["src_row_elems"]
        seen["hop_gt"] += d["hop_elems"] > d["win_row_elems"] or d["hop_rows"] > d["win_rows"]
    assert min(seen.values()) > 20, seen


def test_helpers_build_the_documented_descriptions():
    import microflow_rs_amd as mf
    w = mf.Windows.image((480, 640), (96, 96), 1, 16, n=3)
    assert (w.src_rows, w.src_row_elems, w.win_rows, w.win_row_elems, w.hop_rows, w.hop_elems, w.n_sources) == (480, 640, 96, 96, 16, 16, 3)
    assert w.counts() == (25 * 35, 3 * 25 * 35) and w.stride == 480 * 640
    w = mf.Windows.image((20, 23), (12, 12), 3, (2, 1))
    assert (w.src_row_elems, w.win_row_elems, w.hop_rows, w.hop_elems) == (69, 36, 2, 3) and w.counts() == (5 * 12, 5 * 12)
    w = mf.Windows.frames(64, 40, 49, hop=1)
    assert w.window_elems == 1960 and w.counts() == (16, 16)
    assert mf.Windows.frames(64, 40, 49, hop=2).total == 8


def test_every_invalid_description_is_invalid_arg_and_names_the_field():
    from microflow_rs_amd import _lib
    L = _lib.lib()
    for what, word, d, input_elems, first, count in invalid_descriptions():
        # the gather validates (first, count) and the description; the model entry also the window's size
        st = L.mf_window_gather(0, None, 1, C.byref(desc(d)), first, count, None, None)
        if word != "input_elems":
            assert st == _lib.MF_ERR_INVALID_ARG, what
            assert word in L.mf_last_error().decode(), (what, L.mf_last_error())
        if word not in ("count", "input_elems"):
            assert L.mf_windows_count(C.byref(desc(d)), None, None) == _lib.MF_ERR_INVALID_ARG, what
            assert word in L.mf_last_error().decode(), (what, L.mf_last_error())
    assert L.mf_windows_count(None, None, None) == _lib.MF_ERR_INVALID_ARG
    ok = invalid_descriptions()[0][2]
    assert L.mf_window_gather(0, None, 2, C.byref(desc(dict(ok, hop_rows=1))), 0, 0, None, None) == _lib.MF_ERR_INVALID_ARG
    assert "elem_bytes" in L.mf_last_error().decode()


def test_model_entry_points_validate_before_the_device():
    """on any machine: an unprepared model refuses an invalid description as invalid, whether or not a GPU is there"""
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    L = _lib.lib()
    m = mf.Model(model_path("speech"))      # input_elems 1960
    src = np.zeros(64 * 40, np.int8)
    out = np.zeros(16 * 4, np.int8)
    fout = np.zeros(16 * 4, np.float32)
    good = dict(n_sources=1, src_stride=0, src_rows=64, src_row_elems=40, src_pitch=40, win_rows=49, win_row_elems=40, hop_rows=1, hop_elems=1)
    cases = [("hop_rows", dict(good, hop_rows=0), 0, 1), ("hop_elems", dict(good, hop_elems=0), 0, 1), ("win_rows", dict(good, src_rows=48), 0, 1),
             ("src_pitch", dict(good, src_pitch=39), 0, 1), ("src_stride", dict(good, n_sources=2, src_stride=100), 0, 1),
             ("input_elems", dict(good, win_rows=48), 0, 1), ("count", good, 10, 7)]
    for word, d, first, count in cases:
        for fn, o in (("mf_model_run_windows", out), ("mf_model_predict_quantized_windows", fout)):
            st = getattr(L, fn)(m._h, src.ctypes.data_as(C.c_void_p), C.byref(desc(d)), first, count, o.ctypes.data_as(C.c_void_p), _lib.MF_MEM_HOST)
            assert st == _lib.MF_ERR_INVALID_ARG, (fn, word)
            assert word in L.mf_last_error().decode(), (fn, word, L.mf_last_error())
    fsrc = np.zeros(64 * 40 + 1, np.float32)
    st = L.mf_model_predict_windows(m._h, C.c_void_p(fsrc.ctypes.data + 1), C.byref(desc(good)), 0, 1, fout.ctypes.data_as(C.c_void_p), _lib.MF_MEM_HOST)
    assert st == _lib.MF_ERR_INVALID_ARG and "aligned" in L.mf_last_error().decode()
    both = np.zeros(64 * 40, np.int8)       # src and out must not overlap
    st = L.mf_model_run_windows(m._h, both.ctypes.data_as(C.c_void_p), C.byref(desc(good)), 0, 16, C.c_void_p(both.ctypes.data + 100), _lib.MF_MEM_HOST)
    assert st == _lib.MF_ERR_INVALID_ARG and "overlap" in L.mf_last_error().decode()
    st = L.mf_model_run_windows(m._h, src.ctypes.data_as(C.c_void_p), C.byref(desc(good)), 0, 1, out.ctypes.data_as(C.c_void_p), 7)
    assert st == _lib.MF_ERR_INVALID_ARG
    assert L.mf_model_set_window_chunk(m._h, 5) == _lib.MF_OK and L.mf_model_set_window_chunk(None, 5) == _lib.MF_ERR_INVALID_ARG
    with pytest.raises(mf.MicroflowError) as ei:
        m.run_windows(src, mf.Windows.frames(64, 40, 48))
    assert ei.value.status == _lib.MF_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        m.run_windows(src.view(np.uint8), mf.Windows.frames(64, 40, 49))
    with pytest.raises(ValueError):
        m.run_windows(src[:-1], mf.Windows.frames(64, 40, 49))


def test_valid_call_without_a_gpu_is_no_device():
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    L = _lib.lib()
    if L.mf_device_count() > 0:
        pytest.skip("GPU present")
    m = mf.Model(model_path("speech"))
    w = mf.Windows.frames(64, 40, 49)
    src = np.zeros(64 * 40, np.int8)
    out = np.zeros(16 * 4, np.int8)
    st = L.mf_model_run_windows(m._h, src.ctypes.data_as(C.c_void_p), C.byref(w.desc()), 0, 16, out.ctypes.data_as(C.c_void_p), _lib.MF_MEM_HOST)
    assert st == _lib.MF_ERR_NO_DEVICE and b"no CPU fallback" in L.mf_last_error()
    for call in (lambda: m.run_windows(src, w), lambda: m.predict_windows(src.astype(np.float32), w),
                 lambda: m.predict_quantized_windows(src, w)):
        with pytest.raises(mf.MicroflowError) as ei:
            call()
        assert ei.value.status == _lib.MF_ERR_NO_DEVICE
    st = L.mf_window_gather(0, C.c_void_p(16), 1, C.byref(w.desc()), 0, 16, C.c_void_p(32), None)
    assert st == _lib.MF_ERR_NO_DEVICE
    st = L.mf_window_gather_quantize(0, C.c_void_p(16), C.byref(w.desc()), 0, 16, 0.5, 3, C.c_void_p(32), None)
    assert st == _lib.MF_ERR_NO_DEVICE


def test_new_names_in_header_bindings_and_rust_at_abi_3():
    from microflow_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "microflow_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "microflow-amd", "src", "lib.rs")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\bfn\s+%s\s*\(" % n, rust), n
        assert hasattr(_lib.lib(), n), n
    assert re.search(r"\}\s*mf_windows\s*;", code) and "pub struct mf_windows" in rust
    m = re.search(r"typedef struct \{([^}]*)\}\s*mf_windows;", code)
    assert tuple(re.findall(r"\b(\w+)\s*[,;]", m.group(1))) == FIELDS == tuple(f for f, _ in _lib.WindowsDesc._fields_)
    assert C.sizeof(_lib.WindowsDesc) == 9 * C.sizeof(C.c_size_t)
    assert re.search(r"#define MF_ABI_VERSION 3\b", header) and _lib.lib().mf_abi_version() == 3
    assert re.search(r"pub fn predict_windows\b", rust)


@pytest.fixture(scope="module")
def spec_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("windows_spec")
    exe = str(tmp / "windows_spec_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "microflow_rs_amd", "csrc", "windows_spec.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "windows_spec_main.cpp"), "-o", exe])

    def run(lines):
        path = str(tmp / "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(" ".join(str(int(v)) for v in ln) for ln in lines) + "\n")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(rows) == len(lines)
        return rows
    return run


def test_windows_spec_stand_alone_under_sanitizers(spec_program):
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(11)
    descs = random_descriptions()
    lines, wants = [], []
    for d in descs:
        src = np.arange(source_elems(d), dtype=np.int64)       # element = its own index: the windows hold their source offsets
        win = numpy_windows(d, src)
        total = win.shape[0]
        first = int(rng.integers(0, total))
        count = int(rng.integers(0, total - first + 1))
        idx = sorted({0, total - 1, *rng.integers(0, total, 5).tolist()})
        lines.append([d[f] for f in FIELDS] + [d["win_rows"] * d["win_row_elems"], first, count, len(idx)] + idx)
        wants.append((total, [int(win[i, 0]) for i in idx], first, count, d))
    for row, (total, starts, first, count, d) in zip(spec_program(lines), wants):
        v = [int(t) for t in row.split("#")[0].split()]
        assert v[0] == 0 and v[2] == total and v[1] * d["n_sources"] == total, (row, d)
        assert v[5:] == starts, (row, d)
        if count:   # the span holds every element windows [first, first + count) read
            lo, n = v[3], v[4]
            src = np.arange(source_elems(d), dtype=np.int64)
            used = numpy_windows(d, src)[first: first + count]
            assert lo <= used.min() and used.max() < lo + n <= source_elems(d), (row, d)
    bad = [[d[f] for f in FIELDS] + [ie, first, count, 0] for _, _, d, ie, first, count in invalid_descriptions()]
    for row, (what, word, *_rest) in zip(spec_program(bad), invalid_descriptions()):
        assert int(row.split()[0]) == _lib.MF_ERR_INVALID_ARG and word in row.split("#")[1], (what, row)
    # products that do not fit size_t are refused, not wrapped
    huge = 2 ** 63
    over = [[1, 0, huge, 8, huge, 4, 8, 1, 1, 32, 0, 0, 0], [3, huge, 10, 8, 8, 4, 8, 1, 1, 32, 0, 0, 0], [1, 0, huge, 8, 8, huge // 2, 8, 1, 1, 0, 0, 0, 0]]
    for row in spec_program(over):
        assert int(row.split()[0]) == _lib.MF_ERR_INVALID_ARG and "overflows" in row, row
