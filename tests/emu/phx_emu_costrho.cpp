// Test-only host emulation of the phx C ABI, with the cost-proportional-rho
// entry points (phx_cost_rho_stats, phx_cost_rho_apply, phx_w_absdiff):
// phx_emu_fixer.cpp as it stands (included as text, for emu_ctx) and the three
// functions as plain loops in the kernels' order -- tiles in tile order within
// a node, slots in order within a scenario.
#include "phx_emu_fixer.cpp"

#include <cmath>
#include <limits>

extern "C" {

int emu_phx_cost_rho_stats(emu_ctx* c, const phx_tree_desc* T, const double* cost, const double* x,
                           const double* xbar_node, const int32_t* xbar_idx, const double* denom_node,
                           double* partial, double* scen_denom_out, double* out, void*) {
    if (!c || !T) return 1;
    const int S = c->S, N = c->N, NNS = T->NNS;
    const double ninf = -std::numeric_limits<double>::infinity();
    if (!cost || !out) { c->err = "phx_cost_rho_stats: cost and out required"; return 1; }
    if (!denom_node && !(x && xbar_node && xbar_idx && scen_denom_out)) {
        c->err = "phx_cost_rho_stats: x, xbar_node, xbar_idx and scen_denom_out required without denom_node";
        return 1;
    }
    if (T->ntiles == 0 || T->nnodes_cover != NNS)
        for (int e = 0; e < NNS; ++e) {
            out[e] = out[NNS + e] = 0.0;
            out[2 * NNS + e] = out[3 * NNS + e] = ninf;
        }
    if (T->ntiles == 0 || N == 0 || S == 0) return 0;
    if (!partial) { c->err = "phx_cost_rho_stats: partial required"; return 1; }
    if (!denom_node)
        for (int s = 0; s < S; ++s) {
            double d = 0.0;
            for (int j = 0; j < N; ++j) {
                const double diff = x[ix(c->hs.slot_col[j], s, S)] - xbar_node[xbar_idx[ix(j, s, S)]];
                const volatile double sq = diff * diff;
                d = fmax(d, fmax(fabs(diff), 2.0 * sq));
            }
            scen_denom_out[s] = d;
        }
    const int np = T->npart;
    for (int v = 0; v < T->nnodes; ++v) {
        const int nl = T->node_nlen[v], e0 = T->node_off[v];
        const int t0 = T->node_tile_ptr[v], t1 = T->node_tile_ptr[v + 1];
        for (int t = t0; t < t1; ++t)
            for (int l = 0; l < nl; ++l) {
                const int j = T->tile_slot[t] + l;
                double a = 0.0, hi = ninf, nlo = ninf;
                for (int s = T->tile_s0[t]; s < T->tile_s1[t]; ++s) {
                    const double d = denom_node ? denom_node[e0 + l] : scen_denom_out[s];
                    const double r = d == 0.0 ? -ninf : fabs(cost[ix(j, s, S)]) / d;
                    a += r;
                    hi = fmax(hi, r);
                    nlo = fmax(nlo, -r);
                }
                const int o = T->tile_out[t];
                partial[o + l] = a;
                partial[np + o + l] = hi;
                partial[np + o + nl + l] = nlo;
            }
        const double cnt = (double)(T->tile_s1[t1 - 1] - T->tile_s0[t0]);
        for (int l = 0; l < nl; ++l) {
            double a = 0.0, hi = ninf, nlo = ninf;
            for (int t = t0; t < t1; ++t) {
                const int o = T->tile_out[t];
                a += partial[o + l];
                hi = fmax(hi, partial[np + o + l]);
                nlo = fmax(nlo, partial[np + o + nl + l]);
            }
            out[e0 + l] = a;
            out[NNS + e0 + l] = cnt;
            out[2 * NNS + e0 + l] = hi;
            out[3 * NNS + e0 + l] = nlo;
        }
    }
    return 0;
}

int emu_phx_cost_rho_apply(emu_ctx* c, const phx_tree_desc* T, const phx_cost_rho_opts* o, const double* stats,
                           const int32_t* xbar_idx, double* rho, double* rho_node_out, int32_t* kept_out, void*) {
    if (!c || !T || !o) return 1;
    if (!stats || !xbar_idx || !rho || !rho_node_out || !kept_out) {
        c->err = "phx_cost_rho_apply: stats, xbar_idx, rho, rho_node_out and kept_out required";
        return 1;
    }
    const double alpha = o->order_stat;
    if (!(alpha >= 0.0 && alpha <= 1.0)) {
        c->err = "phx_cost_rho_apply: order_stat outside [0, 1] (0 is the min, 0.5 the average, 1 the max)";
        return 1;
    }
    const int NNS = T->NNS;
    for (int e = 0; e < NNS; ++e) {
        const double cnt = stats[NNS + e];
        const double mean = stats[e] / cnt, hi = stats[2 * NNS + e], lo = -stats[3 * NNS + e];
        double r;
        if (alpha == 0.5) r = mean;
        else if (alpha < 0.5) r = lo + alpha * 2 * (mean - lo);
        else r = (2 * mean - hi) + alpha * 2 * (hi - mean);
        rho_node_out[e] = r;
        kept_out[e] = (cnt > 0.0 && std::isfinite(r)) ? 0 : 1;
    }
    for (int64_t k = 0; k < (int64_t)c->N * c->S; ++k) {
        const int e = xbar_idx[k];
        if (kept_out[e] == 0) rho[k] = rho_node_out[e];
    }
    return 0;
}

int emu_phx_w_absdiff(emu_ctx* c, const double* W, double* W_prev, double* out, void*) {
    if (!c) return 1;
    if (!W || !W_prev || !out) { c->err = "phx_w_absdiff: W, W_prev and out required"; return 1; }
    const int S = c->S;
    double a = 0.0;
    for (int s = 0; s < S; ++s) {
        double d = 0.0;
        for (int j = 0; j < c->N; ++j) {
            const int64_t k = ix(j, s, S);
            d += fabs(W[k] - W_prev[k]);
            W_prev[k] = W[k];
        }
        a += d;
    }
    out[0] = a;
    return 0;
}

}  // extern "C"
