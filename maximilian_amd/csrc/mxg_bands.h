// mxg_bands.h -- the reference's two band analysers over a row of FFT magnitudes as plain arithmetic: maxiBarkScaleAnalyser<double>
// (L/maxiBark.h:24-128, alias maxiBark) and maxiFFTOctaveAnalyzer (L/maxiFFT.h:162-205, L/maxiFFT.cpp:207-300).  L/ = src/libs/.
// No device state: the same text compiles for the host (tests/host_bands.cpp) and for the kernels of bands.hip (K19).  The two
// table builders run on the host only (host libm, as the mel tables of mfcc.hip); every step function is host and device.
//
// What is reproduced is what the reference computes:
//   * the Bark limits: barkScale[i] = hzToBark(bin * sR / bS) with the quotient formed in UNSIGNED INTEGER arithmetic (it truncates),
//     the band edges from the int-truncated currentBand * barkScale[last] / 24 walk, and a 25th limit specSize - 1 (the reference
//     writes it one past its int[24] and reads it back): the last bin is never summed, bands can be empty;
//   * a band sum: a double accumulated bin after bin over float inputs; specific = pow(sum, 0.23) (an empty band: exactly 0);
//     relative = specific / max with max starting at 0 and updated by > (a silent frame: 0 / 0 = NaN in all 24 places, a NaN band is
//     skipped by the compare); total = the 24 values added in order;
//   * the octave map from float arithmetic (span = (sr / 2) / n, increment 2^(1 / perOctave), first band top 55 Hz, perOctave 0 -> 1);
//   * one octave frame, all float, never contracted: sum += x[i] * (intercept + (float)i * slope), count++; when the map value
//     changes at bin i that bin is already in the sum being closed, averages[last .. now) = sum / (float)count, then both reset;
//     the trailing group is written only if its index is below nAverages (it never is: the last map value IS nAverages);
//   * one peak step: avg >= peak takes the average and reloads the hold counter, else the counter counts down, else the peak decays;
//     a NaN average takes the else branch.
// Defined departures: limits the walk never writes are 0 (the reference leaves them uninitialised; only bufferSize 2 and 3 get
// there); a walk that would pass the 25th limit (a top Bark value below 8: sample rates under 2 kHz) stops writing there, where the
// reference overwrites its own specSize; the octave walk gives up past MXG_OCTAVE_MAX_AVERAGES averages.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

#define MXG_BARK_BANDS 24
#define MXG_BARK_MAX_BUFFER 4096     /* the reference's barkScale[2048] */
#define MXG_OCTAVE_MAX_BINS 4096
#define MXG_OCTAVE_MAX_AVERAGES 16384

namespace mxg {
namespace {

// ---- tables (host) ---------------------------------------------------------------------------------------------------------
inline double bnd_hz_to_bark(double hz) { return 13.0 * atan(hz / 1315.8) + 3.5 * atan(pow((hz / 7518.0), 2)); }  // L/maxiBark.h:25-27

// maxiBarkScaleAnalyser::setup (L/maxiBark.h:40-62).  barkScale: bS / 2 doubles of work space.  The caller has checked that
// (bS / 2 - 1) * sR fits 32 bits and bS >= 2.
inline void bnd_bark_limits(unsigned sR, unsigned bS, int lim[MXG_BARK_BANDS + 1], double *barkScale) {
    const unsigned specSize = bS / 2;
    for (unsigned i = 0; i < specSize; i++) barkScale[i] = bnd_hz_to_bark((double)(i * sR / bS));  // binToHz: unsigned, truncating
    for (int b = 0; b <= MXG_BARK_BANDS; b++) lim[b] = 0;
    const double top = barkScale[specSize - 1];
    int currentBandEnd = (int)(top / MXG_BARK_BANDS);
    int currentBand = 1;
    for (unsigned i = 0; i < specSize; i++) {
        while (barkScale[i] > currentBandEnd) {
            if (currentBand <= MXG_BARK_BANDS) lim[currentBand] = (int)i;
            currentBand++;
            currentBandEnd = (int)(currentBand * top / MXG_BARK_BANDS);
        }
    }
    lim[MXG_BARK_BANDS] = (int)specSize - 1;
}

// maxiFFTOctaveAnalyzer::setup (L/maxiFFT.cpp:207-259): spe2avg [nSpectrum]; returns nAverages, or -1 past MXG_OCTAVE_MAX_AVERAGES.
inline int bnd_octave_map(float samplingRate, int nSpectrum, int perOctave, int *spe2avg, float *span_out, float *inc_out) {
    const float span = (samplingRate / 2.0f) / (float)(nSpectrum);
    if (perOctave == 0) perOctave = 1;
    const float inc = powf(2.0f, 1.0f / (float)(perOctave));
    int avgidx = 0;
    float averageFreq = 55.0f;
    float spectrumFreq = span;
    for (int speidx = 0; speidx < nSpectrum; speidx++) {
        while (spectrumFreq > averageFreq) {
            if (++avgidx > MXG_OCTAVE_MAX_AVERAGES) return -1;
            averageFreq *= inc;
        }
        spe2avg[speidx] = avgidx;
        spectrumFreq += span;
    }
    if (span_out) *span_out = span;
    if (inc_out) *inc_out = inc;
    return avgidx;
}

// ---- maxiBark ----------------------------------------------------------------------------------------------------------------
MXG_HD double bnd_bark_add(double sum, float x) { return sum + (double)x; }  // sum += normalisedSpectrum[j]  (:69)

MXG_HD double bnd_bark_band(const float *row, int lo, int hi) {  // one band sum (:66-70)
    double sum = 0;
    for (int j = lo; j < hi; j++) sum = bnd_bark_add(sum, row[j]);
    return sum;
}

MXG_HD double bnd_bark_specific(double sum) {  // (:71)
#if defined(__HIP_DEVICE_COMPILE__)
    // hipcc of ROCm 7.2 does not finish compiling pow() of a value it has traced back to an LDS load (a [64][25] tile read by its
    // lane and passed to pow(x, 0.23) is enough to reproduce it; exp(0.23 * log(x)) or sqrt(x) in its place compile at once).  The
    // empty statement makes the value opaque; it emits no instruction.
    asm volatile("" : "+v"(sum));
#endif
    return pow(sum, 0.23);
}

// v[24]: the band sums in, specificLoudness out; mx = relativeLoudness' max (:87-90), total = totalLoudness (:109-113)
MXG_HD void bnd_bark_loudness(double *v, double &mx, double &total) {
    mx = 0;
    total = 0;
    for (int i = 0; i < MXG_BARK_BANDS; i++) {
        const double s = bnd_bark_specific(v[i]);
        v[i] = s;
        if (s > mx) mx = s;
        total += s;
    }
}

MXG_HD void bnd_bark_relative(double *v, double mx) {  // (:92-94)
    for (int i = 0; i < MXG_BARK_BANDS; i++) v[i] = v[i] / mx;
}

// ---- maxiFFTOctaveAnalyzer -----------------------------------------------------------------------------------------------------
struct OctWalk {
    float sum;
    int count, last;
};

// One bin of calculate() (L/maxiFFT.cpp:266-279).  True when a group closes: averages[from .. to) = avg.
MXG_HD bool bnd_oct_bin(OctWalk &w, float x, int i, int avgidx, float intercept, float slope, float &avg, int &from, int &to) {
    w.count++;
    const float eq = intercept + ((float)(i)*slope);
    w.sum = w.sum + (x * eq);
    const bool closed = avgidx != w.last;
    if (closed) {
        avg = w.sum / (float)(w.count);
        from = w.last;
        to = avgidx;
        w.count = 0;
        w.sum = 0.0f;
    }
    w.last = avgidx;
    return closed;
}

// One frame of calculate() without the peaks (:263-283).
MXG_HD void bnd_octave_frame(const float *row, int nSpectrum, const int *spe2avg, int nAverages, float intercept, float slope,
                             float *averages) {
    OctWalk w = {0.0f, 0, 0};
    for (int i = 0; i < nSpectrum; i++) {
        float avg;
        int from, to;
        if (bnd_oct_bin(w, row[i], i, spe2avg[i], intercept, slope, avg, from, to))
            for (int j = from; j < to; j++) averages[j] = avg;
    }
    if ((w.count > 0) && (w.last < nAverages)) averages[w.last] = w.sum / (float)(w.count);
}

// One band of the peak update (:286-299).
MXG_HD void bnd_peak_step(float avg, float &peak, int32_t &hold, int holdTime, float decay) {
    if (avg >= peak) {
        peak = avg;
        hold = holdTime;
    } else {
        if (hold > 0) hold--;
        else peak = peak * decay;
    }
}

}  // namespace
}  // namespace mxg
