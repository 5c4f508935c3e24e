// windows_spec.cpp -- see windows_spec.hpp.  Host only.
#include "windows_spec.hpp"

namespace mf {

static bool mul(size_t a, size_t b, size_t *r) { return !__builtin_mul_overflow(a, b, r); }
static bool add(size_t a, size_t b, size_t *r) { return !__builtin_add_overflow(a, b, r); }

int windows_check(const mf_windows *w, size_t input_elems, WindowsGeom *g, const char **err) {
    const char *dummy;
    if (!err) err = &dummy;
#define MF_WBAD(msg) return *err = "invalid window description: " msg, (int)MF_ERR_INVALID_ARG
    if (!w || !g) MF_WBAD("null pointer");
    if (w->n_sources == 0) MF_WBAD("n_sources is zero");
    if (w->win_rows == 0 || w->win_row_elems == 0) MF_WBAD("win_rows / win_row_elems is zero");
    if (w->hop_rows == 0) MF_WBAD("hop_rows is zero");
    if (w->hop_elems == 0) MF_WBAD("hop_elems is zero");
    if (w->win_rows > w->src_rows) MF_WBAD("win_rows exceeds src_rows: the window is larger than the source");
    if (w->win_row_elems > w->src_row_elems) MF_WBAD("win_row_elems exceeds src_row_elems: the window is larger than the source");
    if (w->src_pitch < w->src_row_elems) MF_WBAD("src_pitch is shorter than src_row_elems");
    size_t one = 0, win = 0; // elements of one source, from its first to its last; elements of one window
    if (!mul(w->src_rows - 1, w->src_pitch, &one) || !add(one, w->src_row_elems, &one)) MF_WBAD("src_rows * src_pitch overflows");
    if (w->n_sources > 1 && w->src_stride < one) MF_WBAD("src_stride is shorter than one source");
    if (!mul(w->win_rows, w->win_row_elems, &win)) MF_WBAD("win_rows * win_row_elems overflows");
    if (input_elems && win != input_elems) MF_WBAD("win_rows * win_row_elems is not the model's input_elems");
    g->ny = (w->src_rows - w->win_rows) / w->hop_rows + 1;
    g->nx = (w->src_row_elems - w->win_row_elems) / w->hop_elems + 1;
    if (!mul(g->ny, g->nx, &g->per_source) || !mul(g->per_source, w->n_sources, &g->total)) MF_WBAD("the number of windows overflows");
    size_t span = 0;
    if (w->n_sources > 1 && !mul(w->n_sources - 1, w->src_stride, &span)) MF_WBAD("n_sources * src_stride overflows");
    if (!add(span, one, &g->span)) MF_WBAD("n_sources * src_stride overflows");
    *err = "";
    return MF_OK;
}

int windows_range_check(const WindowsGeom &g, size_t first, size_t count, const char **err) {
    const char *dummy;
    if (!err) err = &dummy;
    size_t end = 0;
    if (!add(first, count, &end) || end > g.total) MF_WBAD("first + count is beyond the number of windows");
#undef MF_WBAD
    *err = "";
    return MF_OK;
}

size_t windows_start(const mf_windows &w, const WindowsGeom &g, size_t index) {
    const size_t t = index / g.nx, ix = index - t * g.nx, s = t / g.ny, iy = t - s * g.ny;
    return (w.n_sources > 1 ? s * w.src_stride : 0) + iy * w.hop_rows * w.src_pitch + ix * w.hop_elems;
}

void windows_span(const mf_windows &w, const WindowsGeom &g, size_t first, size_t count, size_t *lo, size_t *n) {
    *lo = 0, *n = 0;
    if (!count) return;
    // whole sources: from the first element of the first window's source to the last element of the last window's
    const size_t s0 = first / g.per_source, s1 = (first + count - 1) / g.per_source;
    const size_t stride = w.n_sources > 1 ? w.src_stride : 0;
    *lo = s0 * stride;
    *n = (s1 - s0) * stride + (w.src_rows - 1) * w.src_pitch + w.src_row_elems;
}

} // namespace mf
