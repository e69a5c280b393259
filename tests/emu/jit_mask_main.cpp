// Stand-alone check of phx_jit.h's fixed_nonant_structure with a slot mask
// (the host code behind phx_fix_nonants_where's fixed-subset lane module),
// meant to be built with -fsanitize=address,undefined and run on its own
// (tests/test_fixer.py does): a small structure, every mask of its slots, and
// the generated source of each.  Exit status 0 when every property holds.
#include <stdio.h>
#include <string.h>
#include "../../mpi-sppy_amd/csrc/phx_jit.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    using namespace phx;
    // 5 columns, 3 rows; columns 0, 2, 3 are nonant slots 0, 1, 2
    HostSetup hs;
    const int n = 5, m = 3;
    hs.rowptr = {0, 3, 5, 7};
    hs.colidx = {0, 1, 4, 1, 2, 3, 4};
    const int nnz = (int)hs.colidx.size();
    hs.kvar.assign(nnz, -1);
    hs.Aconst.assign(nnz, 1.0);
    hs.slot_col = {0, 2, 3};
    const std::string err = build_setup(hs, n, m, nnz, 3, 0, std::vector<double>());
    EXPECT(err.empty());
    EXPECT(hs.col_slot.size() == (size_t)n && hs.col_slot[2] == 1 && hs.col_slot[1] == -1);
    const std::vector<double> lb = {0, 0, 0, -INFINITY, 1}, ub = {10, INFINITY, 10, 5, 1};
    const std::vector<double> bl = {-INFINITY, 0, 2}, bu = {4, 0, INFINITY};
    LaneStructure L;
    std::string why;
    EXPECT(build_lane_structure(hs, n, m, nnz, false, false, false, lb, ub, bl, bu, 1, 1, L, why));
    set_lane_values(L, std::vector<double>(nnz, 1.0), std::vector<double>(n, 1.0), std::vector<double>(m, 1.0),
                    std::vector<double>(n, 1.0), lb, ub, bl, bu);
    EXPECT(L.fixed[4] == 1 && L.fixed[0] == 0 && L.lb.size() == (size_t)n);
    const std::string full = lane_kernel_source(fixed_nonant_structure(L), 2, false);
    for (int bits = 0; bits < 8; ++bits) {
        uint8_t mask[3] = {(uint8_t)(bits & 1), (uint8_t)((bits >> 1) & 1), (uint8_t)((bits >> 2) & 1)};
        const LaneStructure F = fixed_nonant_structure(L, mask);
        EXPECT(F.bnd_vary && F.lb.empty() && F.ub.empty());
        for (int j = 0; j < n; ++j) {
            const int s = hs.col_slot[j];
            if (s >= 0 && mask[s]) {
                EXPECT(F.fixed[j] == 1 && F.lfin[j] == 1 && F.ufin[j] == 1);
            } else {
                EXPECT(F.fixed[j] == L.fixed[j] && F.lfin[j] == L.lfin[j] && F.ufin[j] == L.ufin[j]);
            }
        }
        const std::string src = lane_kernel_source(F, 2, false);
        EXPECT(src.find("bnd_vary() { return true; }") != std::string::npos);
        EXPECT((src == full) == (bits == 7));
    }
    // the input is not modified, and a null mask is every slot
    EXPECT(!L.bnd_vary && L.fixed[0] == 0);
    uint8_t ones[3] = {1, 1, 1};
    EXPECT(lane_kernel_source(fixed_nonant_structure(L, ones), 2, false) == full);
    printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
