// Test-only host emulation of the phx C ABI, with the scenario-donor entry
// points (phx_donor_gather, phx_fix_nonants): phx_emu_rho.cpp as it stands
// (included as text, for emu_ctx) and the two functions as plain loops.
//
// phx_fix_nonants writes the emulation's override arrays, so the emulated solve
// of a fixed problem stays on its generic path (the library runs its
// fixed-nonant lane module: the same answer by another route).  As the library
// does after a generic-path solve, the fixed values are stored into x's nonant
// columns again when the solve returns; for that, and to drop the fixing when
// the bounds are set another way, the three entry points below are the
// included ones under another name plus that bookkeeping.
#define emu_phx_solve emu_phx_solve_plain
#define emu_phx_set_bounds emu_phx_set_bounds_plain
#define emu_phx_destroy emu_phx_destroy_plain
#include "phx_emu_rho.cpp"
#undef emu_phx_solve
#undef emu_phx_set_bounds
#undef emu_phx_destroy

struct EmuFix {
    const double* vals = nullptr;     // node values while nonants are fixed through phx_fix_nonants
    const int32_t* idx = nullptr;
    bool base_ok = false;             // lbs_ovr / ubs_ovr hold the problem's bounds outside the nonant rows
};
static std::map<const emu_ctx*, EmuFix> g_emu_fix;

static void emu_store_fixed(const emu_ctx* c, const EmuFix& f, double* x) {
    const int S = c->S;
    for (int j = 0; j < c->N; ++j)
        for (int s = 0; s < S; ++s) x[ix(c->hs.slot_col[j], s, S)] = f.vals[f.idx[ix(j, s, S)]];
}

extern "C" {

int emu_phx_destroy(emu_ctx* c) {
    g_emu_fix.erase(c);
    return emu_phx_destroy_plain(c);
}

int emu_phx_set_bounds(emu_ctx* c, const double* lb, const double* ub, void* stream) {
    const int rc = emu_phx_set_bounds_plain(c, lb, ub, stream);
    if (rc == 0 && c) {
        EmuFix& f = g_emu_fix[c];
        f.vals = nullptr;
        f.idx = nullptr;
        if (lb) f.base_ok = false;
    }
    return rc;
}

int emu_phx_solve(emu_ctx* c, const phx_solve_opts* o, double* x_out, double* y_out, double* obj_out,
                  int32_t* status_out, int32_t* iters_out, int32_t* total_iters_host, void* stream) {
    const int rc = emu_phx_solve_plain(c, o, x_out, y_out, obj_out, status_out, iters_out, total_iters_host, stream);
    if (rc == 0 && c && x_out) {
        auto it = g_emu_fix.find(c);
        // (an overridden solve is never deferred: x_out is final here)
        if (it != g_emu_fix.end() && it->second.vals && c->bounds_override) emu_store_fixed(c, it->second, x_out);
    }
    return rc;
}

// Test hook: the source of the library's fixed-nonant lane module for this
// context's problem (phx_jit.h fixed_nonant_structure), for the offline
// hipRTC compile check.
const char* emu_phx_fixed_lane_source(const emu_ctx* c, int warm_waves) {
    static std::string src;
    src = c->have_lane ? phx::lane_kernel_source(phx::fixed_nonant_structure(c->ls), warm_waves, false) : std::string();
    return src.c_str();
}

int emu_phx_donor_gather(emu_ctx* c, const phx_tree_desc* T, const double* vals, const int32_t* donor_host,
                         double* out, void*) {
    if (!c || !c->have || !T) { if (c) c->err = "phx_donor_gather: no problem set"; return 1; }
    if (!vals || !out || (!donor_host && T->nnodes)) { c->err = "phx_donor_gather: vals, donor and out required"; return 1; }
    const int S = c->S;
    for (int v = 0; v < T->nnodes; ++v) {
        const int lo = T->tile_s0[T->node_tile_ptr[v]], hi = T->tile_s1[T->node_tile_ptr[v + 1] - 1];
        const int d = donor_host[v];
        if (d != -1 && (d < lo || d >= hi || d >= S)) {
            c->err = "phx_donor_gather: donor " + std::to_string(d) + " of local node " + std::to_string(v) +
                     " is outside the node's local scenarios [" + std::to_string(lo) + ", " + std::to_string(hi) + ")";
            return 1;
        }
    }
    for (int e = 0; e < T->NNS; ++e) out[e] = 0.0;
    for (int v = 0; v < T->nnodes; ++v) {
        const int d = donor_host[v];
        const int j0 = T->tile_slot[T->node_tile_ptr[v]];
        for (int l = 0; l < T->node_nlen[v]; ++l) out[T->node_off[v] + l] = d >= 0 ? vals[ix(j0 + l, d, S)] : 0.0;
    }
    return 0;
}

int emu_phx_fix_nonants(emu_ctx* c, const double* node_vals, const int32_t* xbar_idx, double* x, void* stream) {
    if (!c || !c->have) { if (c) c->err = "phx_fix_nonants: no problem set"; return 1; }
    if (!node_vals) return emu_phx_set_bounds(c, nullptr, nullptr, stream);
    if (c->pend.pending) { c->err = "phx_fix_nonants: a deferred solve is pending (phx_solve_finish)"; return 1; }
    if (!xbar_idx) { c->err = "phx_fix_nonants: xbar_idx required"; return 1; }
    if (c->N <= 0) { c->err = "phx_fix_nonants: the problem has no nonants"; return 1; }
    const int S = c->S, n = c->n;
    EmuFix& f = g_emu_fix[c];
    if (!f.base_ok || c->lbs_ovr.size() != (size_t)n * S) {
        c->lbs_ovr.assign((size_t)n * S, 0.0);
        c->ubs_ovr.assign((size_t)n * S, 0.0);
        for (int j = 0; j < n; ++j)
            for (int s = 0; s < S; ++s) {
                const int64_t src = c->bnd_vary ? ix(j, s, S) : j;
                c->lbs_ovr[ix(j, s, S)] = c->lbs[src];
                c->ubs_ovr[ix(j, s, S)] = c->ubs[src];
            }
        f.base_ok = true;
    }
    for (int j = 0; j < c->N; ++j) {
        const int col = c->hs.slot_col[j];
        for (int s = 0; s < S; ++s) {
            const double v = node_vals[xbar_idx[ix(j, s, S)]];
            const double sv = v / c->hs.dc[col];
            c->lbs_ovr[ix(col, s, S)] = sv;
            c->ubs_ovr[ix(col, s, S)] = sv;
            if (x) x[ix(col, s, S)] = v;
        }
    }
    c->P.lb = SVec{c->lbs_ovr.data(), S, 1};
    c->P.ub = SVec{c->ubs_ovr.data(), S, 1};
    c->bounds_override = true;
    f.vals = node_vals;
    f.idx = xbar_idx;
    return 0;
}

}  // extern "C"
