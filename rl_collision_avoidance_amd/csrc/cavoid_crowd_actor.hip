// cavoid_crowd_actor.hip -- launch of crowd_actor_kernel<NB, RVO> (cavoid_crowd_actor.hpp): cavoid_crowd_actor_run (cavoid_actor.hip) on an env
// of more than kTileMaxAgents agents per world.  Two buckets of the agent count (17..32, 33..64) x (plain, ORCA-carrying env step); N itself
// is a kernel argument.  Own translation unit, compiled with -mllvm -disable-machine-licm like every other step-loop unit (build.py): the
// kernel runs policy + env step + bookkeeping inside one step loop.
#include "cavoid_actor_host.hpp"
#include "cavoid_crowd_actor.hpp"

using namespace cavoid;

int cavoid_launch_crowd_actor(cavoid_env *e, const SplitArgs &sa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                              hipStream_t s) {
    // the env step borrows the (idle) activation planes: crowd_kernel's allocation, at most 64 KB of the planes' 66 KB -- the live mask
    // behind the planes survives it
    unsigned tiles = 0;
    if (int rc_t = crowd_loop_tiles(e, /*lent=*/(size_t)2 * kSpPlaneB, /*refuse_ahead=*/true, &tiles)) return rc_t;
    return dispatch_crowd_bucket(e->cfg.max_agents, e->k.rvo_enabled != 0, [&](auto nb, auto rvo) {
        return launch_big_lds<crowd_actor_kernel<decltype(nb)::value, decltype(rvo)::value>>(
            e->device, policy_split_lds_bytes(), tiles, s, loop_kcfg(e, /*stream_obs=*/true), e->st, (const PoolRec *)e->pool, sa, rc, rs, rio, io, e->cfg.max_agents);
    });
}
