// Test-only host emulation of the phx C ABI, with the adaptive-rho entry
// points (phx_node_absdev, phx_norm_rho, phx_rho_sums): phx_emu.cpp as it
// stands (included as text, for emu_ctx) and the three functions as plain
// loops in the kernels' summation order -- tiles in tile order within a node,
// entries in index order, slots in order within a scenario.
#include "phx_emu.cpp"

extern "C" {

int emu_phx_node_absdev(emu_ctx* c, const phx_tree_desc* T, const double* x, const double* xbar_node,
                        const double* wt, int32_t wt_per_slot, double* partial, double* out, void*) {
    const int S = c->S;
    if (!x || !xbar_node || !wt || !out) { c->err = "phx_node_absdev: x, xbar_node, wt and out required"; return 1; }
    if (T->ntiles > 0 && !partial) { c->err = "phx_node_absdev: partial required"; return 1; }
    for (int e = 0; e <= T->NNS; ++e) out[e] = 0.0;
    for (int v = 0; v < T->nnodes; ++v) {
        const int nl = T->node_nlen[v], e0 = T->node_off[v];
        for (int t = T->node_tile_ptr[v]; t < T->node_tile_ptr[v + 1]; ++t)
            for (int l = 0; l < nl; ++l) {
                const int j = T->tile_slot[t] + l;
                const int col = c->hs.slot_col[j];
                double a = 0;
                for (int s = T->tile_s0[t]; s < T->tile_s1[t]; ++s) {
                    const double w = wt_per_slot ? wt[ix(j, s, S)] : wt[s];
                    a += w * fabs(x[ix(col, s, S)] - xbar_node[e0 + l]);
                }
                partial[T->tile_out[t] + l] = a;
            }
        for (int l = 0; l < nl; ++l) {
            double a = 0;
            for (int t = T->node_tile_ptr[v]; t < T->node_tile_ptr[v + 1]; ++t) a += partial[T->tile_out[t] + l];
            out[e0 + l] = a;
        }
    }
    double tot = 0;
    for (int e = 0; e < T->NNS; ++e) tot += out[e];
    out[T->NNS] = tot;
    return 0;
}

int emu_phx_norm_rho(emu_ctx* c, const phx_tree_desc* T, const phx_norm_rho_opts* o, const double* primal,
                     const double* xbar_node, double* xbar_prev, const int32_t* xbar_idx, double* rho,
                     double* dual_out, int32_t* action_out, void*) {
    const int S = c->S;
    if (!o || !primal || !xbar_node || !xbar_prev || !xbar_idx || !rho || !action_out) {
        c->err = "phx_norm_rho: primal, xbar_node, xbar_prev, xbar_idx, rho and action_out required";
        return 1;
    }
    for (int e = 0; e < T->NNS; ++e) {
        action_out[e] = 0;
        if (dual_out) dual_out[e] = 0.0;
    }
    for (int v = 0; v < T->nnodes; ++v) {
        const int tl = T->node_tile_ptr[v + 1] - 1;
        const int s_last = T->tile_s1[tl] - 1;
        for (int l = 0; l < T->node_nlen[v]; ++l) {
            const int e = T->node_off[v] + l;
            const double p = primal[e];
            const double d = rho[ix(T->tile_slot[tl] + l, s_last, S)] * fabs(xbar_node[e] - xbar_prev[e]);
            int act = 0;
            if (p > o->pd_factor * d && p > o->tol) {
                act = 1;
            } else if (d > o->pd_factor * p && d > o->tol) {
                if (o->allow_decrease) act = 2;
            } else if (p < o->tol && d < o->tol) {
                act = 3;
            }
            action_out[e] = act;
            if (dual_out) dual_out[e] = d;
            xbar_prev[e] = xbar_node[e];
        }
    }
    for (int64_t k = 0; k < (int64_t)c->N * S; ++k) {
        const int act = action_out[xbar_idx[k]];
        if (act == 1) rho[k] = rho[k] * o->rho_increase;
        else if (act == 2) rho[k] = rho[k] / o->rho_decrease;
        else if (act == 3) rho[k] = rho[k] / o->conv_decrease;
    }
    return 0;
}

int emu_phx_rho_sums(emu_ctx* c, const double* rho, const double* prob, const double* xbar_node,
                     const double* xbar_prev, const int32_t* xbar_idx, double* out, void*) {
    const int S = c->S;
    if (!rho || !prob || !out || (xbar_prev && !(xbar_node && xbar_idx))) {
        c->err = "phx_rho_sums: rho, prob and out required (xbar_node and xbar_idx with xbar_prev)";
        return 1;
    }
    double a = 0, b = 0;
    for (int s = 0; s < S; ++s) {
        double r = 0, d = 0;
        for (int j = 0; j < c->N; ++j) {
            const int64_t k = ix(j, s, S);
            r += rho[k];
            if (xbar_prev) d += rho[k] * fabs(xbar_node[xbar_idx[k]] - xbar_prev[xbar_idx[k]]);
        }
        a += prob[s] * r;
        b += d;
    }
    out[0] = a;
    out[1] = b;
    return 0;
}

}  // extern "C"
