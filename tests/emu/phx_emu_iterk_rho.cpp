// Test-only host emulation of the phx C ABI, with phx_iterk_norm_rho:
// phx_emu_costrho.cpp as it stands (included as text, for emu_ctx and the
// entry points it chains) and the device loop with the norm-rho update restated
// sequentially -- emu_phx_iterk's loop with emu_phx_node_absdev /
// emu_phx_norm_rho between the convergence sums and the stop test (the
// reference's miditer, phbase.py:914-926), and the same adoption of a pending
// deferred Iter0.
#include "phx_emu_costrho.cpp"

extern "C" {

int emu_phx_iterk_norm_rho(emu_ctx* c, const phx_solve_opts* o, const phx_iterk_args* a, phx_iterk_rho* ra,
                           phx_iterk_result* res, void* stream) {
    if (!c || !c->have || !o || !a || !res) { if (c) c->err = "phx_iterk: bad arguments"; return 1; }
    if (!ra) { c->err = "phx_iterk_norm_rho: rho_args required"; return 1; }
    if (!ra->prob || !ra->partial || !ra->primal || !ra->xbar_prev || !ra->action_out) {
        c->err = "phx_iterk_norm_rho: prob, partial, primal, xbar_prev and action_out required";
        return 1;
    }
    if (!o->sp && c->sp_ok) {
        c->err = "phx_iterk: sp = 0 asks for the dense generic path, which this problem's context does not hold "
                 "(its subproblems are served by the sparse solver)";
        return 1;
    }
    if (c->pend.pending) emu_adopt_pending(c);
    const bool adopted = c->adopted;
    c->adopted = false;
    if (adopted) {
        if (a->iter0_obj) for (int s = 0; s < c->S; ++s) a->iter0_obj[s] = c->pend.obj_out[s];
        if (a->iter0_status && c->pend.status_out)
            for (int s = 0; s < c->S; ++s) a->iter0_status[s] = c->pend.status_out[s];
        if (a->iter0_obj && a->iter0_status && a->iter0_prob && a->iter0_expect && a->iter0_expect_host) {
            emu_phx_expect(c, a->iter0_prob, a->iter0_obj, a->iter0_status, a->iter0_expect, nullptr);
            for (int k = 0; k < 3; ++k) a->iter0_expect_host[k] = a->iter0_expect[k];
        }
    }
    const bool lane_mode = o->lane_solver && c->have_lane && !c->bounds_override && c->solved_once;
    const bool wg_mode = !lane_mode && !(o->lane_solver && c->have_lane) && c->wg_ok && o->wg_warm > 0 &&
                         o->polish && o->warm_start && c->solved_once && !c->bounds_override;
    const bool sp_mode = !lane_mode && !wg_mode && !(o->lane_solver && c->have_lane) && c->sp_ok && o->sp &&
                         o->polish && o->warm_start && c->solved_once && !c->bounds_override;
    if (!(lane_mode || wg_mode || sp_mode)) {
        c->err = "phx_iterk: needs the lane solver, the workgroup warm pass or the sparse solver, after a first "
                 "solve and no bound override";
        return 1;
    }
    if (!(a->tree && a->node_sums && a->node_stage && a->nseg > 0 && a->conv_R == a->nseg)) {
        c->err = "phx_iterk: missing arrays";
        return 1;
    }
    *res = phx_iterk_result{};
    res->adopted = adopted ? 1 : 0;
    res->adopted_stragglers = adopted ? c->adopt_stragglers : 0;
    ra->updates = 0;
    const int NNS = a->tree->NNS;
    if (adopted) {
        double nbad = (double)c->stats_adopted.not_optimal + (double)c->stats_adopted.infeasible;
        if (a->allreduce) {
            a->node_stage[2 * NNS] = nbad;
            if (a->allreduce(a->allreduce_user, a->node_stage, 2 * (int64_t)NNS + 1, stream)) {
                c->err = "phx_iterk: all-reduce of the Iter0 not-optimal count failed";
                return 1;
            }
            nbad = a->node_stage[2 * NNS];
        }
        if (nbad > 0.0) {
            res->not_optimal = c->stats_adopted.not_optimal;
            c->stats_override = true;
            return 0;
        }
    }
    phx_solve_opts o2 = *o;
    o2.defer = 0;
    double* rho = const_cast<double*>(a->rho);
    for (int k = 1; k <= a->max_iters; ++k) {
        emu_phx_xbar(c, a->tree, a->x, a->prob_coeff, a->partial, a->node_stage, stream);
        a->node_stage[2 * NNS] = 0.0;
        if (a->allreduce && a->allreduce(a->allreduce_user, a->node_stage, 2 * (int64_t)NNS + 1, stream)) {
            c->err = "phx_iterk: all-reduce failed";
            return 1;
        }
        for (int e = 0; e < 2 * NNS; ++e) a->node_sums[e] = a->node_stage[e];
        emu_phx_update_w(c, a->x, a->node_sums, a->xbar_idx, a->rho, a->W, a->W, 1, nullptr, a->nseg,
                         a->seg_s0_host, a->seg_s1_host, a->seg_sums, stream);
        if (a->allreduce && a->allreduce(a->allreduce_user, a->seg_sums, a->nseg, stream)) {
            c->err = "phx_iterk: all-reduce failed";
            return 1;
        }
        double tot = 0.0;
        for (int r = 0; r < a->conv_R; ++r)
            if (a->conv_counts_host[r] > 0) tot += a->seg_sums[r] / a->conv_counts_host[r];
        const double conv = tot / a->conv_R;
        res->iters = k;
        res->conv = conv;
        // miditer: before the stop test, so the iteration that converges updates too
        if (!(ra->stop_after_iter >= 0 && k > ra->stop_after_iter)) {
            if (!ra->have_prev) {
                for (int e = 0; e < NNS; ++e) ra->xbar_prev[e] = a->node_sums[e];
                ra->have_prev = 1;
            } else {
                if (emu_phx_node_absdev(c, a->tree, a->x, a->node_sums, ra->prob, 0, ra->partial, ra->primal, stream))
                    return 1;
                if (a->allreduce && a->allreduce(a->allreduce_user, ra->primal, (int64_t)NNS + 1, stream)) {
                    c->err = "phx_iterk_norm_rho: all-reduce of the primal residuals failed";
                    return 1;
                }
                phx_norm_rho_opts ro = ra->opts;
                ro.allow_decrease = k >= ra->decrease_from_iter ? 1 : 0;
                if (emu_phx_norm_rho(c, a->tree, &ro, ra->primal, a->node_sums, ra->xbar_prev, a->xbar_idx, rho,
                                     ra->dual_out, ra->action_out, stream))
                    return 1;
                if (ra->action_log)
                    for (int e = 0; e < NNS; ++e) ra->action_log[(int64_t)(k - 1) * NNS + e] = ra->action_out[e];
                ra->updates += 1;
            }
        }
        if (conv < a->convthresh) { res->converged = 1; break; }
        int32_t total = 0;
        // W / xbar / rho moved in place: refresh the generic path's PH terms
        emu_phx_set_ph_terms(c, c->ph_W, c->ph_rho, c->ph_xbar, c->ph_idx, c->ph_W_on, c->ph_prox_on, stream);
        if (emu_phx_solve(c, &o2, a->x, a->y, a->obj, a->status, a->iters, &total, stream)) return 1;
        res->solves += 1;
        res->stragglers += c->S - c->lane_certified;
        res->not_optimal = c->not_optimal;
    }
    if (adopted) c->stats_override = true;       // phx_last_solve_stats: the adopted solve's
    return 0;
}

}  // extern "C"
