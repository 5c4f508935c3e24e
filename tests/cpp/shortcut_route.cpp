// shortcut_route.cpp -- what the grouping rules ask of a parsed model with side operators, without a device (tests/test_shortcut_host.py):
// links against libmicroflow_amd.so, parses the .tflite files named on the command line and prints, per file,
//   side <i> <source> ...            every side operator and the operator it reads (-1: the model input)
//   add <i> <skip_src> <skip_real> <candidate>   every ADD: the tensor it reads, the operator whose tensor stays in memory for it,
//                                    and the side operator rule (6b) would group with it (-1: none)
//   span <first> <last> <0|1>        for every pair first <= last: would one launch over first .. last be refused (group_splits)?
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "model_groups.hpp"

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        try {
            const mf::ParsedModel pm = mf::parse_tflite(bytes.data(), bytes.size());
            std::printf("file %s %zu\n", argv[a], pm.ops.size());
            for (size_t i = 0; i < pm.ops.size(); ++i) {
                if (pm.ops[i].side()) std::printf("side %zu %d\n", i, pm.ops[i].side_src);
                if (pm.ops[i].kind == MF_OP_ADD) std::printf("add %zu %d %d %d\n", i, pm.ops[i].skip_src, pm.skip_real(i), mf::side_join_candidate(pm, i));
            }
            for (size_t i = 0; i < pm.ops.size(); ++i)
                for (size_t j = i; j < pm.ops.size(); ++j) std::printf("span %zu %zu %d\n", i, j, mf::group_splits(pm, i, j) ? 1 : 0);
            std::printf("forks %zu %d\n", pm.max_fork_elems, pm.input_skip ? 1 : 0);
        } catch (const mf::Error &e) {
            std::printf("error %d %s\n", e.code, e.msg.c_str());
            return 1;
        }
    }
    return 0;
}
