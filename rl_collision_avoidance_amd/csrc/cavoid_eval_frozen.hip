// cavoid_eval_frozen.hip -- eval_kernel<N, true, true> (cavoid_eval.hpp): the evaluation loop for worlds that hold frozen-network agents
// (scripted policy 4) -- the env step's 'everything' instantiation plus a second forward pass on the frozen network's weights for the tiles
// that hold a running one.  Own translation unit (compile time; built with -mllvm -disable-machine-licm like cavoid_eval.hip).
#include "cavoid_eval_host.hpp"

using namespace cavoid;

int cavoid_launch_eval_frozen(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const EvalIO &io, hipStream_t s) {
    return launch_eval_any<true, true>(e, sa, fz, io, s);
}
