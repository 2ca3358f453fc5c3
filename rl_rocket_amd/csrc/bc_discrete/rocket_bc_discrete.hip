// rocket_bc_discrete.hip — the tenth translation unit of librocket_hip.so: behaviour cloning of the
// Categorical policy on the device (rr_bc_update_discrete), what imitation's bc.BC does per minibatch
// for SB3's MlpPolicy over Discrete(K) (the reference's keyboard demonstrations are indices into
// DiscreteActions3DOF's table):
//   log p_ik = z_ik - logsumexp_k z_ik,  logp_i = log p_{i, a_i},  H_i = -sum_k p_ik log p_ik
//   loss     = -mean_i logp_i - ent_weight mean_i H_i + l2_weight 0.5 sum_{all 12 tensors} w^2
//   Adam (capturable, no clip) over the 12 tensors.
// The kernels (bcd_*) and their launch sequence are rocket_bc.inc's with RR_BC_DISCRETE 1, over
// discrete/rocket_discrete.hip's <7, 4> images, the choices K = 2 .. 4 a runtime count. Launched through
// rrc_launch_bc_discrete with a BcLaunch that has n_choices and a sink. Compiled with the collect
// translation unit's settings (build.py COLLECT_FLAGS), because the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"
#define RR_BC_DISCRETE 1
#include "rocket_bc.inc"

// rr_bc_update_discrete's launches (declared in rocket_device.h); `launch` points to the BcLaunch of the
// calling TU.
extern "C" int rrc_launch_bc_discrete(const void* launch, void* stream)
{
    return bc_launch<7, 4>(from_unit<BcLaunch>(launch), (hipStream_t)stream);
}
