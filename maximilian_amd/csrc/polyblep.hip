// polyblep.hip -- maxiPolyBLEP banks on gfx950 (K20): the reference's anti-aliased oscillator (src/libs/maxiPolyBLEP.h over
// src/libs/PolyBLEP/PolyBLEP.cpp), fourteen waveforms over one phase recurrence per voice.  The per-sample arithmetic is
// mxg_polyblep.h, which also compiles for the host (mxg_polyblep_host below, tests/host_polyblep.cpp).
//
// polyblep_kernel has the streaming shape of mxg_stream.h: one lane = one voice, chunks of 8 samples, surplus lanes shadow the
// last voice (pair) and store no phase, whole chunks leave through emit_chunk (8-byte stores or 16-byte pair rows), a ragged last
// chunk by 8-byte stores, per-sample frequency rows are requested a chunk ahead.  The waveform is a template argument: a launch
// has one waveform, so no lane ever branches on it.  What a lane does branch on is the data: the arms of blep / blamp, the
// piecewise waveforms and the fallback to a sine at freq >= sr / 4.
// HBM per sample: 8 B out (+ 8 B with per-sample frequencies); per voice 8 B phase in and out, 8 B frequency, 8 B pulse width.
// LDS: the 16 KB sin / cos table of mxg_sincos.h, in every instantiation (the fallback is a sine whatever the waveform).
// No scratch.
#include <math.h>

#include "mxg_common.h"
#include "mxg_stream.h"
#include "mxg_polyblep.h"

namespace mxg {
namespace {

__device__ const double MXG_PB_SINTAB_D[MXG_SINTAB_LEN] = {MXG_SINTAB_VALUES};
const double kPbSinTabHost[MXG_SINTAB_LEN] = {MXG_SINTAB_VALUES};

struct PbArgs {
    size_t V, N;
    const double *pw;  // [V] or null: 0.5
    double sr;
    double *t;  // [V] in / out
    int px_store;
};

// FPS: a frequency block [N][V]; else one frequency per voice [V].  freq / out are separate __restrict__ parameters, as in envgen.hip.
template <int WF, bool FPS, bool PX>
__global__ void __launch_bounds__(256) polyblep_kernel(PbArgs A, const double *__restrict__ freq, double *__restrict__ out_ptr) {
    __shared__ double s_tab[MXG_SINTAB_LEN];
    for (int i = threadIdx.x; i < MXG_SINTAB_LEN; i += blockDim.x) s_tab[i] = MXG_PB_SINTAB_D[i];
    __syncthreads();
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const bool live = gid < V;
    const size_t v = bank_voice<PX>(gid, V);
    double t = A.t[v], pw = A.pw ? A.pw[v] : 0.5, f0 = FPS ? 0.0 : freq[v];
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(t), "+v"(pw), "+v"(f0));
    const PbSinTab sc = {s_tab, sintab_k()};
    const double sr = A.sr;
    constexpr int U = 8;
    const double *__restrict__ fp = FPS ? freq + v : nullptr;
    double *op = out_ptr + v;
    double fn[U];
    if constexpr (FPS) rows_first(fn, fp, V, N);
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double fc[U];
        if constexpr (FPS) {
            rows_next(fc, fn, fp, V, N, n0);
        } else {
#pragma unroll
            for (int i = 0; i < U; i++) fc[i] = f0;
        }
        const int cnt = n0 + U <= N ? U : (int)(N - n0);  // (wave-uniform, mxg_stream.h)
        double y[U];
#pragma unroll
        for (int i = 0; i < U; i++) {
            y[i] = pb_play<WF>(t, fc[i], sr, pw, sc);
            if (i + 1 == cnt) break;
        }
        emit_rows<PX>(op, V, y, cnt, A.px_store);
    }
    if (!live) return;  // a shadow lane owns no phase
    A.t[v] = t;
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_polyblep_host(int waveform, size_t V, size_t N, const double *h_freq, int fps, const double *h_pw, double sample_rate,
                      double *h_t, double *h_out) {
    MXG_REQUIRE(V > 0 && N > 0, "V and N must be at least 1");
    MXG_REQUIRE(waveform >= 0 && waveform < MXG_PBLEP_WAVEFORMS, "waveform is not one of MXG_PBLEP_*");
    MXG_REQUIRE(sample_rate > 0, "sample_rate must be positive");
    MXG_REQUIRE(h_freq, "h_freq is null");
    MXG_REQUIRE(h_t, "h_t is null");
    MXG_REQUIRE(h_out, "h_out is null");
    const PbSinTab sc = {kPbSinTabHost, {1.0 / 120, 1.0 / 24}};
    pb_dispatch(waveform, [&](auto WF) {
        for (size_t v = 0; v < V; v++) {
            double t = h_t[v];
            const double pw = h_pw ? h_pw[v] : 0.5;
            for (size_t n = 0; n < N; n++) h_out[n * V + v] = pb_play<WF.value>(t, h_freq[fps ? n * V + v : v], sample_rate, pw, sc);
            h_t[v] = t;
        }
    });
    return MXG_OK;
}

int mxg_polyblep_render(int waveform, size_t V, size_t N, const double *d_freq, int fps, const double *d_pw, double sample_rate,
                        double *d_t, double *d_out, void *stream) {
    MXG_REQUIRE(V > 0 && N > 0, "V and N must be at least 1");
    MXG_REQUIRE(waveform >= 0 && waveform < MXG_PBLEP_WAVEFORMS, "waveform is not one of MXG_PBLEP_*");
    MXG_REQUIRE(sample_rate > 0, "sample_rate must be positive");
    MXG_REQUIRE(d_freq, "d_freq is null");
    MXG_REQUIRE(d_t, "d_t is null");
    MXG_REQUIRE(d_out, "d_out is null");
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    const int block = voice_block(V, true);
    const PbArgs A = {V, N, d_pw, sample_rate, d_t, rw_store_choice(V, N, d_out, fps ? RW_READ_WRITE : RW_WRITE_ONLY)};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("polyblep_kernel", st);
    pb_dispatch(waveform, [&](auto WF) {
        with_bools([&](auto FPS, auto PX) {
            hipLaunchKernelGGL((polyblep_kernel<WF.value, FPS.value, PX.value>), voice_grid(V, block), dim3(block), 0, st, A, d_freq, d_out);
        }, fps != 0, A.px_store != 0);
    });
    return check_hip(hipGetLastError(), "polyblep_kernel launch");
}

}  // extern "C"
