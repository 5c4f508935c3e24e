// model_groups.hpp -- what model_prepare builds for a parsed model (model_groups.cpp) and the model runtime launches (model.cpp):
// the prepared operators, the first-level groups over them and the second-level stages over those.
#pragma once
#include <utility>
#include <vector>

#include "mf_internal.hpp"

namespace mf {

// The single owner of all three tiers.  Move-only; destroys stages first, then first-level groups, then operators.
struct ModelGroups {
    std::vector<OpImpl *> ops; // nullptr for Reshape
    // fused[i] != nullptr: ops i .. fused_last[i] run as ONE kernel (depthwise + 1x1 conv pairs;
    // the pool -> head conv -> [reshape] -> softmax tail)
    std::vector<FusedImpl *> fused;
    std::vector<int> fused_last;
    // second level: ops first .. last (several first-level groups / operators) as ONE kernel: a run of identical pair
    // groups (k_stage.hip), a one-input-channel depthwise + FullyConnected + Softmax (k_dwfc.hip), the last pair + the
    // tail (k_tail3.hip).  They do not overlap; what is inside stays available for mf_model_run_until.
    struct Stage {
        FusedImpl *f;
        int first, last;
    };
    std::vector<Stage> stages;
    // side_join[i] != nullptr: join i -- an ADD or a CONCATENATION -- and the side operator whose output it reads
    // (ParsedModel::side_of_join) run as ONE launch at the join's index (k_side_join.hip).  The one group whose members need not be
    // neighbours in file order, and the one with two inputs
    std::vector<FusedImpl *> side_join;
    // the first / last operator that launches anything (leading Reshapes alias the input -- speech.tflite starts with one --
    // trailing ones the output): ops.size() / -1 where there is none
    int first_real = 0, last_real = -1;

    ModelGroups() = default;
    ModelGroups(const ModelGroups &) = delete;
    ModelGroups &operator=(const ModelGroups &) = delete;
    ModelGroups(ModelGroups &&o) noexcept { swap(o); }
    ModelGroups &operator=(ModelGroups &&o) noexcept {
        swap(o);
        return *this;
    }
    ~ModelGroups() { clear(); }
    void clear(); // stages borrow the groups' buffers, groups the operators': in that order
    void swap(ModelGroups &o) noexcept {
        ops.swap(o.ops), fused.swap(o.fused), fused_last.swap(o.fused_last), stages.swap(o.stages), side_join.swap(o.side_join);
        std::swap(first_real, o.first_real), std::swap(last_real, o.last_real);
    }
};

// What the rules ask of the parsed model alone (host only; tests/cpp/shortcut_route.cpp and concat_route.cpp print them):
// would operators first .. last as ONE launch swallow a tensor that has to exist in memory, a join (ADD, CONCATENATION), or a side operator?
bool group_splits(const ParsedModel &pm, size_t first, size_t last);
// rule (6b) by everything the file says: the side operator that forms one launch with join `join` -- shortcut_add_rt with an ADD,
// side_concat_rt with a CONCATENATION (geometry, filter zero points in the i8 domain, finite constants: shortcut_add_class /
// side_concat_class) -- or -1: no join, no side operator there, or one outside the class
int side_join_candidate(const ParsedModel &pm, size_t join);
// (the same question under the names it had per kind of join, which route printers written against earlier trees still call)
inline int shortcut_candidate(const ParsedModel &pm, size_t add) { return pm.ops[add].kind == MF_OP_ADD ? side_join_candidate(pm, add) : -1; }
inline int side_concat_candidate(const ParsedModel &pm, size_t join) { return pm.ops[join].kind == MF_OP_CONCATENATION ? side_join_candidate(pm, join) : -1; }
bool shortcut_add_class(const OpSpec &conv, bool zero_wzp, bool finite);                  // (fused_heads.hip)
bool side_concat_class(const OpSpec &conv, int run_channels, bool zero_wzp, bool finite); // (fused_heads.hip)

// Operators and every group the grouping rules find, built in a local: a failure half way (a HIP error, OOM, a geometry an
// operator rejects) destroys what exists and throws.  autotune: time the run-time-geometry chain candidates on the device
ModelGroups build_groups(const ParsedModel &pm, int device, bool autotune);

} // namespace mf
