// cavoid_multistep.hip -- the env_kernel instantiations that take several auto-reset steps inside ONE launch
// (cavoid_step_autoreset_n / cavoid_step_autoreset_packed with n_steps > 1): MODE_STEP_AUTORESET_PF (small batches: the next
// scenario-pool record of every lane is held in registers) and MODE_STEP_AUTORESET_N (restarts gather on demand).
// Own translation unit because it is compiled with -mllvm -disable-machine-licm (build.py): MachineLICM would hoist every
// constant materialisation of the step body out of the step loop into registers live across it.
#include "cavoid_launch.hpp"

using namespace cavoid;

int cavoid_launch_multistep(cavoid_env *e, const KIO &io, bool prefetch, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (relay_form_first(e, io, prefetch)) {                            // small batch: the step cut into roles on several wavefronts (env_relay_kernel)
        const int rc = cavoid_launch_relay(e, io, s, ev_start, ev_stop);   // (records its own form: it knows the consumer count)
        // (io.ahead_hi: the look-ahead rings were prepared for the relay form with its top-up wavefront -- no other form may run on them)
        if (rc != CAVOID_EUNSUPPORTED || io.ahead_hi) return rc;
    } else if (io.ahead_hi) {
        return CAVOID_EINVAL;
    }
    if (crowd_form(e->cfg.max_agents))                                  // more than kTileMaxAgents agents per world: the crowd form's step loop
        return note_form(e, cavoid_launch_crowd(e, MODE_STEP_AUTORESET_N, e->k, e->st, e->W, io, s, ev_start, ev_stop), crowd_step_form(e));
    if (e->k.rvo_enabled || (e->k.gen_mode == 1 && e->k.pool_size <= 0))       // ORCA agents / in-step box generator: cavoid_rvo.hip
        return cavoid_launch_rvo(e, prefetch ? MODE_STEP_AUTORESET_PF : MODE_STEP_AUTORESET_N, io, s, ev_start, ev_stop);
    // (continuous actions: the role-split and pipelined forms decode table actions only -- the single-wavefront loops carry them)
    if (prefetch && e->pipeline && !io.cont) {                          // two wavefronts per tile, pipelined (env_pipe_kernel)
        const int rc = launch_pipe<false>(e, io, s, ev_start, ev_stop);
        if (rc != CAVOID_EUNSUPPORTED) return note_form(e, rc, CAVOID_FORM_PIPE);
    }
    if (prefetch) return note_form(e, launch_on<MODE_STEP_AUTORESET_PF>(e, e->k, e->st, e->grid, io, s, ev_start, ev_stop), CAVOID_FORM_LOOP_PF);
    return note_form(e, launch_on<MODE_STEP_AUTORESET_N>(e, e->k, e->st, e->grid, io, s, ev_start, ev_stop), CAVOID_FORM_LOOP);
}

#ifdef CAVOID_TRACE
int cavoid_debug_trace_multistep(unsigned long long *dev_ptr) { return set_trace(dev_ptr); }
#endif
