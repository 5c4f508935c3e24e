// windows_spec.hpp -- the host arithmetic of an mf_windows description (include/microflow_amd.h, section 5): validation, counts and
// the source element a window starts at.  No HIP and no other part of the library: windows_spec.cpp compiles alone with a host
// compiler (tests/test_windows_host.py runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <stddef.h>

#include "../../include/microflow_amd.h"

namespace mf {

struct WindowsGeom {
    size_t ny = 0, nx = 0;   // windows per source: down, across
    size_t per_source = 0;   // ny * nx
    size_t total = 0;        // n_sources * per_source
    size_t span = 0;         // elements from the first element of source 0 to the last element of the last source, inclusive
};
// MF_OK, or MF_ERR_INVALID_ARG with *err naming the offending field (a static string).  input_elems = 0: the window's size is not
// compared with a model's.  Every product the description implies is checked for overflow of size_t.
int windows_check(const mf_windows *w, size_t input_elems, WindowsGeom *g, const char **err);
// first + count inside the total
int windows_range_check(const WindowsGeom &g, size_t first, size_t count, const char **err);
// source element of element (0, 0) of window `index` (index < g.total)
size_t windows_start(const mf_windows &w, const WindowsGeom &g, size_t index);
// elements from the first source element windows [first, first + count) read to the last, inclusive: [*lo, *lo + *n)
void windows_span(const mf_windows &w, const WindowsGeom &g, size_t first, size_t count, size_t *lo, size_t *n);

} // namespace mf
