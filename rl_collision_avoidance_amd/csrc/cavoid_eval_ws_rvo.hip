// cavoid_eval_ws_rvo.hip -- eval_ws_kernel<N, true> (cavoid_eval_ws.hpp): the weight-sharing evaluation loop over the env step's ORCA
// instantiation -- worlds with scripted RVO agents (and the envs cavoid_actor_run_ws routes there).  Own translation unit (compile time;
// built with -mllvm -disable-machine-licm like cavoid_eval_ws.hip).
#include "cavoid_eval_ws_host.hpp"

using namespace cavoid;

int cavoid_launch_eval_ws_rvo(cavoid_env *e, const PolicyWsArgs &wa, const EvalIO &io, hipStream_t s) { return launch_eval_ws_any<true>(e, wa, wa, io, s); }
