// scan_long_swept_host.cpp -- the host build of mxg_scan_long_swept.h inside the library: what mxg_scan_long_swept_host runs.  Plain
// C++ (not a HIP translation unit), so the shared text compiles as ordinary host functions.
#include <new>
#include <vector>

#include "mxg_scan_long_swept.h"

namespace mxg {

// 0, 1 for a kind without a swept form, 2 when the work array cannot be allocated
int scan_long_swept_host_render(int kind, size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out) {
    std::vector<double> work;
    try {
        work.resize((kSweptPairDoubles + kSweptEndDoubles) * (N / kSweptChunk) + 1);
    } catch (const std::bad_alloc &) {
        return 2;
    }
    return scan_long_swept_host_run(kind, V, N, in, coef, rows, st, out, work.data());
}

}  // namespace mxg
