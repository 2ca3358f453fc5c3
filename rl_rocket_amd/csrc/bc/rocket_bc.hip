// rocket_bc.hip — the eighth translation unit of librocket_hip.so: behaviour cloning on the device
// (rr_bc_update), what imitation's bc.BC does per minibatch for SB3's MlpPolicy with a diagonal
// Gaussian:
//   logp_i  = sum_a (-(a_ia - mean_ia)^2 / (2 std_a^2) - log_std_a - 0.5 log 2 pi)
//   loss    = -mean_i logp_i - ent_weight entropy + l2_weight 0.5 sum_{all 13 tensors} w^2
//   Adam (capturable, no clip) over the 13 tensors.
// The kernels (bc_*) and their launch sequence are rocket_bc.inc's with RR_BC_DISCRETE 0. Launched
// through rrc_launch_bc with a BcLaunch. Compiled with the collect translation unit's settings
// (build.py COLLECT_FLAGS), because the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"
#define RR_BC_DISCRETE 0
#include "rocket_bc.inc"

// rr_bc_update's launches (declared in rocket_device.h); `launch` points to the BcLaunch of the
// calling TU.
extern "C" int rrc_launch_bc(const void* launch, void* stream)
{
    const auto L = from_unit<BcLaunch>(launch);
    return L.obs_dim == 14 ? bc_launch<14, 3>(L, (hipStream_t)stream) : bc_launch<7, 2>(L, (hipStream_t)stream);
}
