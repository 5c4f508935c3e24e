// The MF_CHAIN_PLAN parser (microflow_rs_amd/csrc/switches.cpp) without a GPU: every argument is parsed as a plan and answered with
// one line, `ok len:G:dbuf,...` (the segments as parsed) or `bad <reason>`; then the plan the environment holds, as switches_parse()
// sees it (`env unset`, `env ok ...` or `env bad ...`).  tests/test_chain_plan_host.py builds this under the sanitizers.
#include <cstdio>
#include <string>
#include <vector>
#include "mf_switches.hpp"

static void answer(const char *prefix, bool ok, const std::vector<mf::ChainPlanSeg> &segs, const std::string &err) {
    if (!ok) {
        printf("%sbad %s\n", prefix, err.c_str());
        return;
    }
    printf("%sok ", prefix);
    for (size_t i = 0; i < segs.size(); ++i) printf("%s%d:%d:%d", i ? "," : "", segs[i].len, segs[i].G, segs[i].dbuf);
    printf("\n");
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        std::vector<mf::ChainPlanSeg> segs;
        std::string err;
        const bool ok = mf::chain_plan_parse(argv[i], segs, err);
        if (ok != err.empty() || (!ok && !segs.empty())) return 2; // (a refused plan leaves no segments and says why)
        answer("", ok, segs, err);
    }
    const mf::Switches s = mf::switches_parse();
    if (!s.chain_plan_set) printf("env unset\n");
    else answer("env ", s.chain_plan_error.empty(), s.chain_plan, s.chain_plan_error);
    return 0;
}
