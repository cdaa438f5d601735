// mxg_hd.h -- how a shared "step header" (mxg_*.h: the per-sample arithmetic of a bank family) says where its functions run.
// A step header is compiled three ways: by hipcc's device pass (the kernels), by hipcc's host pass or a plain C++ translation
// unit of the library (the _host twins, e.g. mxg_drum_host, grainpool_host.cpp), and by g++ (the CPU checkers tests/host_*.cpp).
// This header is the whole vocabulary: every step header includes it first and defines no qualifier macro of its own, so what a
// function's qualifier means depends neither on the include order nor on a flag of the translation unit.  No HIP include here.
// Under a plain C++ compiler all three macros are `inline` (not `static inline`): that form also fits a member function, an unused
// inline function draws no -Wunused-function, and a function outside an anonymous namespace is the same token sequence in every
// translation unit that sees it (this header is its only definition), which is what the one-definition rule asks.
#pragma once
#if defined(__HIPCC__)

// MXG_HD: callable on the host and on the device.  For plain arithmetic; a body may fork on __HIP_DEVICE_COMPILE__ for a device
// form of the same operation (a builtin, inline asm) as long as the other branch is ordinary C++.
#define MXG_HD __host__ __device__ __forceinline__
// MXG_DEV: device-only under hipcc.  For whatever cannot exist on hipcc's host pass -- inline asm, __builtin_amdgcn_*, lane
// operations, LDS, HIP's device-only functions such as __double_as_longlong -- and for whatever calls such a function.
#define MXG_DEV __device__ __forceinline__
// MXG_HD_NOINLINE: MXG_DEV without the forced inlining, for a body too large to copy into each of its callers (advance_until).
#define MXG_HD_NOINLINE __device__

#else  // a plain C++ compiler: ordinary inline functions, and stand-ins for what HIP and mxg_common.h provide under hipcc

#include <string.h>
#define MXG_HD inline
#define MXG_DEV inline
#define MXG_HD_NOINLINE inline

#define MXG_TWOPI 6.283185307179586476925286766559
#define MXG_PI 3.1415926535897932384626433832795
inline long long __double_as_longlong(double x) { long long b; memcpy(&b, &x, 8); return b; }
inline double __longlong_as_double(long long b) { double x; memcpy(&x, &b, 8); return x; }
namespace mxg {
constexpr double kChandiv = 1.0;  // C:53 `float chandiv = 1;` (as mxg_common.h)
}

#endif
