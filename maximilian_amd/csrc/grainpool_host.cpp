// grainpool_host.cpp -- the host build of mxg_grainpool.h inside the library: what mxg_granular_pool_host and
// mxg_stretch_loop_host run.  Plain C++ (not a HIP translation unit), so the shared text compiles as ordinary host functions.
#include "mxg_grainpool.h"

namespace mxg {

int grainpool_host_render(int mode, const GpArgs &A) { return gp_host_render(mode, A); }

const char *grainpool_stretch_loop(uint64_t len, double start01, double end01, uint64_t *loopStart, uint64_t *loopEnd) {
    return gp_stretch_loop(len, start01, end01, loopStart, loopEnd);
}

}  // namespace mxg
