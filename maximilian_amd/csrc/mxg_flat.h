// mxg_flat.h -- the skeleton of the FLAT stream kernels (shaper.hip: shape / xfade / select; classic.hip: map): streams without a
// recurrence over time run over the E = N * V elements of a block instead of one lane per voice.  A thread takes kFlatUnits units
// a workgroup's width apart, a unit being 16 bytes (two neighbouring elements, whatever rows they are in) where every pointer is
// 16-byte aligned and the knob rw_store is not 1, else one 8-byte element.  Per-voice parameters are indexed by element % V: one
// remainder per thread (flat_voice0), then stepped by the host-computed remainder of the stride (flat_next).
#pragma once
#include "mxg_common.h"

namespace mxg {
namespace {

constexpr int kFlatBlock = 256;  // threads of a flat workgroup
constexpr int kFlatUnits = 4;    // units per thread

struct FlatGeom {
    size_t E, V;
    unsigned stride_mod;  // (kFlatBlock * elements per unit) % V
    int st;               // store flavour of the 16-byte units: 1 / 2 / 3 = plain / write-through / non-temporal (emit_chunk's numbering)
};

__device__ __forceinline__ void flat_store2(double *p, double a, double b, int st) {
    if (st == 2) store2<2>(p, a, b);
    else if (st == 3) store2<1>(p, a, b);
    else store2<0>(p, a, b);
}

// element % V for the first element of a thread's first unit
__device__ __forceinline__ size_t flat_voice0(size_t e, size_t V) {
    if (V <= 0xffffffffu && e <= 0xffffffffu) return (uint32_t)e % (uint32_t)V;
    return e % V;
}
__device__ __forceinline__ size_t flat_next(size_t m, size_t step, size_t V) {
    m += step;
    return m >= V ? m - V : m;
}

template <bool VEC>
__device__ __forceinline__ void flat_load(const double *p, size_t e, double (&x)[VEC ? 2 : 1]) {
    if constexpr (VEC) {
        const double2v r = *reinterpret_cast<const double2v *>(p + e);
        x[0] = r.x;
        x[1] = r.y;
    } else {
        x[0] = p[e];
    }
}
template <bool VEC>
__device__ __forceinline__ void flat_store(double *p, size_t e, const double (&y)[VEC ? 2 : 1], int st) {
    if constexpr (VEC) flat_store2(p + e, y[0], y[1], st);
    else p[e] = y[0];
}

// the flavour of a flat launch: 16-byte units where every pointer allows it (`all` = the OR of their addresses) and the knob
// rw_store is not 1 (the 8-byte stores); blocks from 64 MB take the write-through stores (mxg_common.h, rw_store_choice)
inline FlatGeom flat_geom(size_t V, size_t N, uintptr_t all, bool *vec) {
    const size_t E = V * N;
    int rw = tune_get("rw_store");
    if (rw == 0) rw = E * sizeof(double) >= ((size_t)64 << 20) ? 3 : 2;
    *vec = rw >= 2 && !(all & 15);
    const size_t stride = (size_t)kFlatBlock * (*vec ? 2 : 1);
    return {E, V, (unsigned)(stride % V), *vec ? rw - 1 : 0};
}
inline unsigned flat_grid(const FlatGeom &g, bool vec) {
    const size_t units = vec ? g.E >> 1 : g.E, per = (size_t)kFlatBlock * kFlatUnits;
    const size_t blocks = (units + per - 1) / per;
    return (unsigned)(blocks ? blocks : 1);  // (E == 1 in 16-byte units: the block that takes the odd element)
}

}  // namespace
}  // namespace mxg
