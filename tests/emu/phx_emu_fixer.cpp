// Test-only host emulation of the phx C ABI, with the Fixer entry points
// (phx_fixer_step, phx_fix_nonants_where): phx_emu_xhat.cpp as it stands
// (included as text, for emu_ctx and its fixing state) and the two functions
// as plain loops.
//
// phx_fix_nonants_where writes the emulation's override arrays, so the emulated
// solve of a partly fixed problem stays on its generic path (the library runs
// its fixed-subset lane module: the same answer by another route).  As the
// library does after a generic-path solve, the fixed values are stored into x's
// fixed columns again when the solve returns.  For that the included solve
// entry point is declared ahead with another linker name and the one below
// takes its place (the included file undefines the macros it renames with, so
// a macro cannot do it).  The partial fixing is on while the included state
// has the index array set and no values: the included phx_set_bounds,
// phx_fix_nonants and phx_destroy end it without knowing of it.
#include "../../include/phx.h"
struct emu_ctx;
extern "C" {
int emu_phx_solve(emu_ctx* c, const phx_solve_opts* o, double* x_out, double* y_out, double* obj_out,
                  int32_t* status_out, int32_t* iters_out, int32_t* total_iters_host, void* stream)
    __asm__("emu_phx_solve_xhat");
int emu_phx_solve_fixer(emu_ctx* c, const phx_solve_opts* o, double* x_out, double* y_out, double* obj_out,
                        int32_t* status_out, int32_t* iters_out, int32_t* total_iters_host, void* stream)
    __asm__("emu_phx_solve");
}
#include "phx_emu_xhat.cpp"

struct EmuWhere {
    const double* vals = nullptr;     // node values and flags while fixed through phx_fix_nonants_where
    const int32_t* fixed = nullptr;
};
static std::map<const emu_ctx*, EmuWhere> g_emu_where;

static const EmuWhere* emu_where_on(const emu_ctx* c) {
    auto f = g_emu_fix.find(c);
    auto w = g_emu_where.find(c);
    if (f == g_emu_fix.end() || w == g_emu_where.end()) return nullptr;
    return c->bounds_override && !f->second.vals && f->second.idx && w->second.vals ? &w->second : nullptr;
}

extern "C" {

int emu_phx_solve_fixer(emu_ctx* c, const phx_solve_opts* o, double* x_out, double* y_out, double* obj_out,
                        int32_t* status_out, int32_t* iters_out, int32_t* total_iters_host, void* stream) {
    const int rc = emu_phx_solve(c, o, x_out, y_out, obj_out, status_out, iters_out, total_iters_host, stream);
    if (rc == 0 && c && x_out) {
        // (an overridden solve is never deferred: x_out is final here)
        if (const EmuWhere* w = emu_where_on(c)) {
            const int S = c->S;
            const int32_t* idx = g_emu_fix[c].idx;
            for (int j = 0; j < c->N; ++j)
                for (int s = 0; s < S; ++s) {
                    const int e = idx[ix(j, s, S)];
                    if (w->fixed[e] != 0) x_out[ix(c->hs.slot_col[j], s, S)] = w->vals[e];
                }
        }
    }
    return rc;
}

// Test hook: the source of the library's fixed-subset lane module for this
// context's problem and slot mask ([N] bytes; phx_jit.h fixed_nonant_structure),
// for the offline hipRTC compile check.
const char* emu_phx_subset_lane_source(const emu_ctx* c, const uint8_t* mask, int warm_waves) {
    static std::string src;
    src = c->have_lane ? phx::lane_kernel_source(phx::fixed_nonant_structure(c->ls, mask), warm_waves, false)
                       : std::string();
    return src.c_str();
}

int emu_phx_fixer_step(emu_ctx* c, int32_t NNS, const double* xbar_node, const double* xsqbar_node,
                       const double* th, const int32_t* nb, const int32_t* lbk, const int32_t* ubk,
                       const double* ent_lb, const double* ent_ub, double boundtol, int32_t iter0, int32_t* count,
                       int32_t* fixed, double* fix_val, int32_t* nfixed_host, void*) {
    if (!c) return 1;
    if (NNS < 0) { c->err = "phx_fixer_step: negative NNS"; return 1; }
    if (NNS > 0 && !(xbar_node && xsqbar_node && th && nb && lbk && ubk && ent_lb && ent_ub && count && fixed &&
                     fix_val)) {
        c->err = "phx_fixer_step: every table and state array is required";
        return 1;
    }
    int32_t nnew = 0;
    for (int e = 0; e < NNS; ++e) {
        if (fixed[e] != 0) continue;
        const double xb = xbar_node[e];
        const volatile double sq = xb * xb;          // (rounded before the subtraction)
        const double diff = sq - xsqbar_node[e];
        const double th2 = th[e] * th[e];
        const bool conv = -diff < th2 && diff < th2;
        int fx = 0;
        if (!iter0) {
            fx = conv ? count[e] + 1 : 0;
            count[e] = fx;
        }
        if (iter0 ? !conv : fx <= 0) continue;
        int how = 0;
        double v = 0.0;
        if (nb[e] >= 0 && (iter0 || nb[e] <= fx)) {
            how = 1;
            v = xb;
        } else if (lbk[e] >= 0 && (iter0 || lbk[e] < fx) && xb - ent_lb[e] < boundtol) {
            how = 2;
            v = ent_lb[e];
        } else if (ubk[e] >= 0 && (iter0 || ubk[e] < fx) && ent_ub[e] - xb < boundtol) {
            how = 3;
            v = ent_ub[e];
        }
        if (how) {
            fixed[e] = how;
            fix_val[e] = v;
            ++nnew;
        }
    }
    if (nfixed_host) *nfixed_host = nnew;
    return 0;
}

int emu_phx_fix_nonants_where(emu_ctx* c, const double* node_vals, const int32_t* node_fixed,
                              const int32_t* xbar_idx, const uint8_t*, double* x, void* stream) {
    if (!c || !c->have) { if (c) c->err = "phx_fix_nonants_where: no problem set"; return 1; }
    if (!node_vals) return emu_phx_set_bounds(c, nullptr, nullptr, stream);
    if (c->pend.pending) { c->err = "phx_fix_nonants_where: a deferred solve is pending (phx_solve_finish)"; return 1; }
    if (!node_fixed || !xbar_idx) { c->err = "phx_fix_nonants_where: node_fixed and xbar_idx required"; return 1; }
    if (c->N <= 0) { c->err = "phx_fix_nonants_where: the problem has no nonants"; return 1; }
    const int S = c->S, n = c->n;
    // the problem's scaled bounds everywhere, then the fixed entries over them
    c->lbs_ovr.assign((size_t)n * S, 0.0);
    c->ubs_ovr.assign((size_t)n * S, 0.0);
    for (int j = 0; j < n; ++j)
        for (int s = 0; s < S; ++s) {
            const int64_t src = c->bnd_vary ? ix(j, s, S) : j;
            c->lbs_ovr[ix(j, s, S)] = c->lbs[src];
            c->ubs_ovr[ix(j, s, S)] = c->ubs[src];
        }
    for (int j = 0; j < c->N; ++j) {
        const int col = c->hs.slot_col[j];
        for (int s = 0; s < S; ++s) {
            const int e = xbar_idx[ix(j, s, S)];
            if (node_fixed[e] == 0) continue;
            const double v = node_vals[e];
            const double sv = v / c->hs.dc[col];
            c->lbs_ovr[ix(col, s, S)] = sv;
            c->ubs_ovr[ix(col, s, S)] = sv;
            if (x) x[ix(col, s, S)] = v;
        }
    }
    c->P.lb = SVec{c->lbs_ovr.data(), S, 1};
    c->P.ub = SVec{c->ubs_ovr.data(), S, 1};
    c->bounds_override = true;
    EmuFix& f = g_emu_fix[c];
    f.vals = nullptr;                 // (not the included all-nonant store: emu_where_on)
    f.idx = xbar_idx;
    f.base_ok = true;
    g_emu_where[c] = EmuWhere{node_vals, node_fixed};
    return 0;
}

}  // extern "C"
