// scan_long_host.cpp -- the host build of mxg_scan_long.h inside the library: what mxg_scan_long_host runs.  Plain C++ (not a HIP
// translation unit), so the shared text compiles as ordinary host functions.
#include <new>
#include <vector>

#include "mxg_scan_long.h"

namespace mxg {

// 0, 1 for an unknown kind, 2 when the work array cannot be allocated
int scan_long_host_render(int kind, size_t V, size_t N, const double *in, const double *coef, double *st, double *out) {
    std::vector<double> work;
    try {
        work.resize(6 * (N / kLongChunk) + 1);
    } catch (const std::bad_alloc &) {
        return 2;
    }
    return scan_long_host_run(kind, V, N, in, coef, st, out, work.data());
}

}  // namespace mxg
