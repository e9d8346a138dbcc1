// Host build of d3ga_amd/csrc/perceptual_math.h for tests/test_perceptual_host.py: the packing maps of the 3x3 convolution's
// weight panels.  Both panels are filled the way pc_pack_kernel fills them -- every slot asks pc_panel_source where its
// eight elements come from -- and then read back through the forward map pc_panel_elem.
#include <cstdint>
#include <vector>

#include "../../d3ga_amd/csrc/perceptual_math.h"

using namespace d3ga;

static std::vector<int64_t> fill(int w_cout, int w_cin, int transposed) {
    const int64_t slots = transposed ? pc_plane_slots(w_cout, w_cin) : pc_plane_slots(w_cin, w_cout);
    std::vector<int64_t> panel(slots * 8);
    for (int64_t s = 0; s < slots; ++s)
        for (int j = 0; j < 8; ++j) panel[s * 8 + j] = pc_panel_source(w_cout, w_cin, transposed, s, j);
    return panel;
}

extern "C" {

// number of violations for a weight tensor (w_cout, w_cin, 3, 3); 0 passes
int64_t pc_check_panels(int w_cout, int w_cin) {
    const std::vector<int64_t> fwd = fill(w_cout, w_cin, 0), bwd = fill(w_cout, w_cin, 1);
    int64_t bad = 0;
    if ((int64_t)fwd.size() * 2 * kVggPlanes != pc_panel_bytes(w_cin, w_cout)) ++bad;
    if ((int64_t)bwd.size() * 2 * kVggPlanes != pc_panel_bytes(w_cout, w_cin)) ++bad;
    for (int co = 0; co < w_cout; ++co)
        for (int ci = 0; ci < w_cin; ++ci)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const int64_t src = (((int64_t)co * w_cin + ci) * 3 + ky) * 3 + kx;
                    // forward GEMM (w_cin -> w_cout): output co, input ci, tap (ky, kx)
                    if (fwd[pc_panel_elem(w_cin, w_cout, co, ci, ky, kx)] != src) ++bad;
                    // input-gradient GEMM (w_cout -> w_cin): the forward slot of (ci, co, 2 - ky, 2 - kx)
                    if (bwd[pc_panel_elem(w_cout, w_cin, ci, co, 2 - ky, 2 - kx)] != src) ++bad;
                }
    // every other slot is K or N padding: zero
    int64_t used_f = 0, used_b = 0;
    for (int64_t v : fwd) used_f += v >= 0;
    for (int64_t v : bwd) used_b += v >= 0;
    if (used_f != (int64_t)w_cout * w_cin * 9) ++bad;
    if (used_b != (int64_t)w_cout * w_cin * 9) ++bad;
    return bad;
}

int64_t pc_host_panel_bytes(int cin, int cout) { return pc_panel_bytes(cin, cout); }
int pc_host_ksteps(int cin) { return pc_ksteps(cin); }

}
