// mxg_svf.h -- one sample of maxiSVF::play(w, lpmix, bpmix, hpmix, notchmix) (H:1305-1319, H = src/maximilian.h): the Cytomic
// trapezoidal state-variable filter as plain arithmetic over its three state values.  c = g1, g2, g3, g4, k (maxiSVF::setParams,
// evaluated on the host libm by mxg_svf_coeffs_host) followed by the four mix arguments.  + - * only, the reference's expression
// trees: bit-exact.  The same text compiles for the host and the device: the hats of mxg_drums.h (K21).  filter2.hip's SVF bank keeps
// the same statements inline in its two kernels: calling this function from them gives the same bits but another instruction
// schedule, and that kernel's device listing is held fixed.
#pragma once

#include "mxg_hd.h"

namespace mxg {
namespace {

MXG_HD double svf_step(double &v0z, double &v1, double &v2, double x, const double (&c)[9]) {
    const double v1z = v1;
    const double v2z = v2;
    const double v3 = x + v0z - 2.0 * v2z;
    v1 += c[0] * v3 - c[1] * v1z;
    v2 += c[2] * v3 + c[3] * v1z;
    v0z = x;
    const double low = v2, band = v1;
    const double high = x - c[4] * v1 - v2;
    const double notch = x - c[4] * v1;
    return (low * c[5]) + (band * c[6]) + (high * c[7]) + (notch * c[8]);
}

}  // namespace
}  // namespace mxg
