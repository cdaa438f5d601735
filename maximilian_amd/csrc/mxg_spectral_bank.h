// mxg_spectral_bank.h -- the integer arithmetic maxiFFTBank / maxiIFFTBank (spectral_bank.hip, kernel K29) share between the host
// and the device: where a call's frames and consumption points fall, and which row of spectra a point of the inverse bank takes.
// Plain C++ over mxg_hd.h: the library's host code, the kernels and mxg_spectral_bank_plan_host run this one text.
#pragma once
#include <stddef.h>

#include "mxg_hd.h"

namespace mxg {

// What a call of N samples does to V maxiFFT / maxiIFFT objects in lock-step.  One counter serves a whole bank, because it depends
// only on the sequence of N values:
//   fill = maxiFFT's pos - (windowSize - hopSize), 0 <= fill < hop: samples taken since the last frame (L/maxiFFT.cpp:67-87)
//   pos  = maxiIFFT's pos, 0 <= pos < hop (L/maxiFFT.cpp:155-189)
struct SpectralBankPlan {
    size_t frames;      // frames every maxiFFT completes inside the call (pos == windowSize, :69)
    size_t points;      // samples of the call at which every maxiIFFT transforms a spectrum (0 == pos, :155)
    int first_is_held;  // after-FFT rows: point 0 takes the spectrum held from the call before (the call starts ON a point)
    int new_fill, new_pos;
};

MXG_HD SpectralBankPlan spectral_bank_plan(int hop, int fill, int pos, size_t N) {
    SpectralBankPlan p;
    const size_t H = (size_t)hop;
    p.frames = ((size_t)fill + N) / H;
    p.new_fill = (int)(((size_t)fill + N) % H);
    // multiples of hop in [pos, pos + N)
    p.points = ((size_t)pos + N + H - 1) / H - ((size_t)pos + H - 1) / H;
    p.new_pos = (int)(((size_t)pos + N) % H);
    p.first_is_held = (pos == 0 && p.points > 0) ? 1 : 0;
    return p;
}

// The consumption point and the offset inside its hop of sample n of a call entered at `pos`.  Point -1 is the frame consumed
// before the call: its samples come out of the carried buffer.
MXG_HD void spectral_bank_sample(int hop, int pos, size_t n, long long *point, int *offset) {
    const size_t t = (size_t)pos + n;
    *point = (long long)(t / (size_t)hop) - (pos > 0 ? 1 : 0);
    *offset = (int)(t % (size_t)hop);
}

// Row of spectra that consumption point j takes.  direct rows: row j.  after-FFT rows (the rows a maxiFFTBank of the same hop,
// created at the same time, emitted for the same N): frame k completes at global sample k * hop + hop - 1 and is consumed at
// (k + 1) * hop, so a call entered between two points (pos > 0) finds point j's frame in row j, and a call entered ON a point
// (pos == 0) in row j - 1, row -1 being the held spectrum.
MXG_HD long long spectral_bank_row(int after_fft, int first_is_held, size_t j) {
    return (long long)j - ((after_fft && first_is_held) ? 1 : 0);
}

// Element index of row r (frame / point f of stream v) of a block of `per` rows per stream: layout 0 = frame-major, 1 = stream-major.
MXG_HD size_t spectral_bank_row_index(int layout, size_t V, size_t per, size_t v, size_t f) {
    return layout ? v * per + f : f * V + v;
}

}  // namespace mxg
