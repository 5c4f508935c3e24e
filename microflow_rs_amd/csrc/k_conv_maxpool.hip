// k_conv_maxpool.hip -- a Conv2D and the MaxPool2D behind it in one launch: conv_pool_rt (k_conv_pool.hip) with phase B taking the max
// of the in-range dwords of Y instead of their masked v_dot4 sums, from the same text (k_conv_pool_body.inc).  Steps, phases, plan
// (k::conv_pool_plan), bands, barriers and LDS layout are DESIGN 4.17's; the pool's arithmetic is maxpool_generic's (DESIGN section 2:
// the max over the in-range taps only, then average_pool_2d.rs:56 on that one byte).  A translation unit of its own so that
// k_conv_pool.hip keeps exactly its 36 instances.
#include "k_common.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

#define MF_CONV_POOL_KERNEL conv_maxpool_rt
#define MF_CONV_POOL_MAX 1
#define MF_CONV_POOL_LAUNCH launch_conv_maxpool
#define MF_CONV_POOL_LAUNCH_T launch_conv_maxpool_t
#define MF_CONV_POOL_LAUNCH_W launch_conv_maxpool_w
#include "k_conv_pool_body.inc"

} // namespace k
} // namespace mf
