// cavoid_actor_ws_rvo.hip -- actor_ws_kernel<N, true> (cavoid_actor_ws.hpp): the weight-sharing network's fused actor loop over the env
// step's ORCA instantiation -- worlds with scripted RVO agents, and box scenarios (GEN v2) generated inside the step.  Own translation
// unit (compile time; built with -mllvm -disable-machine-licm like cavoid_actor_ws.hip).
#include "cavoid_actor_ws_host.hpp"

using namespace cavoid;

int cavoid_launch_actor_ws_rvo(cavoid_env *e, const PolicyWsArgs &wa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                               hipStream_t s) {
    return launch_actor_ws_any<true>(e, wa, rc, rs, rio, io, s);
}
