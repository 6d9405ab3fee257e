// cavoid_eval_ws_frozen.hip -- eval_ws_kernel<N, true, true> (cavoid_eval_ws.hpp): the weight-sharing evaluation loop for worlds that hold
// frozen-network agents (scripted policy 4) -- the env step's 'everything' instantiation plus a second row-list pass on the frozen
// network's weights for the tiles that hold a running one.  Own translation unit (compile time; built with -mllvm -disable-machine-licm
// like cavoid_eval_ws.hip).
#include "cavoid_eval_ws_host.hpp"

using namespace cavoid;

int cavoid_launch_eval_ws_frozen(cavoid_env *e, const PolicyWsArgs &wa, const PolicyWsArgs &fz, const EvalIO &io, hipStream_t s) {
    return launch_eval_ws_any<true, true>(e, wa, fz, io, s);
}
