// cavoid_eval_rvo.hip -- eval_kernel<N, true> (cavoid_eval.hpp): the evaluation loop over the env step's ORCA instantiation -- worlds with
// scripted RVO agents (and the envs cavoid_actor_run routes there).  Own translation unit (compile time; built with
// -mllvm -disable-machine-licm like cavoid_eval.hip).
#include "cavoid_eval_host.hpp"

using namespace cavoid;

int cavoid_launch_eval_rvo(cavoid_env *e, const SplitArgs &sa, const EvalIO &io, hipStream_t s) { return launch_eval_any<true>(e, sa, sa, io, s); }
