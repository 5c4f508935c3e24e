// windows_spec_main.cpp -- stand-alone driver of microflow_rs_amd/csrc/windows_spec.cpp for tests/test_windows_host.py, built with
// the host compiler under the address and undefined-behaviour sanitizers.
//
//   windows_spec_main <cases.txt>
//
// Every line of the file is one description and one request:
//   n_sources src_stride src_rows src_row_elems src_pitch win_rows win_row_elems hop_rows hop_elems input_elems first count k i_0 .. i_{k-1}
// and is answered on stdout with
//   status per_source total span_lo span_n start(i_0) .. start(i_{k-1})
// (status 0: everything else is valid; otherwise the numbers are 0 and the message follows on the same line after a '#').
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../microflow_rs_amd/csrc/windows_spec.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s cases.txt\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    for (;;) {
        unsigned long long v[13];
        int got = 0;
        for (; got < 13; ++got)
            if (fscanf(f, "%llu", &v[got]) != 1) break;
        if (got == 0) break;
        if (got != 13) return fprintf(stderr, "short line\n"), 2;
        std::vector<size_t> idx((size_t)v[12]);
        for (size_t &i : idx) {
            unsigned long long t;
            if (fscanf(f, "%llu", &t) != 1) return fprintf(stderr, "short index list\n"), 2;
            i = (size_t)t;
        }
        mf_windows w;
        w.n_sources = (size_t)v[0], w.src_stride = (size_t)v[1], w.src_rows = (size_t)v[2], w.src_row_elems = (size_t)v[3];
        w.src_pitch = (size_t)v[4], w.win_rows = (size_t)v[5], w.win_row_elems = (size_t)v[6], w.hop_rows = (size_t)v[7];
        w.hop_elems = (size_t)v[8];
        mf::WindowsGeom g;
        const char *err = "";
        int st = mf::windows_check(&w, (size_t)v[9], &g, &err);
        if (st == MF_OK) st = mf::windows_range_check(g, (size_t)v[10], (size_t)v[11], &err);
        if (st != MF_OK) {
            printf("%d 0 0 0 0", st);
            for (size_t k = 0; k < idx.size(); ++k) printf(" 0");
            printf(" # %s\n", err);
            continue;
        }
        size_t lo = 0, n = 0;
        mf::windows_span(w, g, (size_t)v[10], (size_t)v[11], &lo, &n);
        printf("0 %zu %zu %zu %zu", g.per_source, g.total, lo, n);
        for (size_t i : idx) printf(" %zu", i < g.total ? mf::windows_start(w, g, i) : (size_t)0);
        printf("\n");
    }
    fclose(f);
    return 0;
}
