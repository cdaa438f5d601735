// tools/gen/bands_ref_dump.cpp -- TEST INFRASTRUCTURE (tools/gen/gen_golden_bands.py).  The UNMODIFIED reference's
// maxiBarkScaleAnalyser<double> (src/libs/maxiBark.h) and maxiFFTOctaveAnalyzer (src/libs/maxiFFT.h / .cpp) behind a C interface
// for ctypes.  Compiled with -fno-access-control: the Bark limits are private, and the 25th one is read back from where the
// reference wrote it, one past its int[24].  The octave analyser's public arrays, which the reference leaves uninitialised, are
// zeroed after setup().
#include <string.h>

#include "maxiBark.h"
#include "maxiFFT.h"

extern "C" {

// limits [25] as the object holds them after setup(); specific / relative [nframes][24], total [nframes]
void bnd_ref_bark(unsigned sR, unsigned bS, float *spec, size_t stride, size_t nframes, int *limits, double *specific, double *relative,
                  double *total) {
    static maxiBark obj;  // (static storage, as a patch declares it: the write one past bbLimits lands in the object's next member)
    maxiBark *b = &obj;
    b->setup(sR, bS);
    volatile int *lim = b->bbLimits;
    for (int i = 0; i <= 24; i++) limits[i] = lim[i];
    for (size_t f = 0; f < nframes; f++) {
        memcpy(specific + f * 24, b->specificLoudness(spec + f * stride), sizeof(double) * 24);
        memcpy(relative + f * 24, b->relativeLoudness(spec + f * stride), sizeof(double) * 24);
        total[f] = b->totalLoudness(spec + f * stride)[0];
    }
}

void *bnd_ref_octave_new(float sr, int n, int perOctave) {
    maxiFFTOctaveAnalyzer *o = new maxiFFTOctaveAnalyzer();
    o->setup(sr, n, perOctave);
    for (int i = 0; i < o->nAverages; i++) {
        o->averages[i] = 0.0f;
        o->peaks[i] = 0.0f;
        o->peakHoldTimes[i] = 0;
    }
    return o;
}

int bnd_ref_octave_info(void *h, int *map) {
    maxiFFTOctaveAnalyzer *o = (maxiFFTOctaveAnalyzer *)h;
    if (map) memcpy(map, o->spe2avg, sizeof(int) * o->nSpectrum);
    return o->nAverages;
}

void bnd_ref_octave_calc(void *h, float *mags, size_t stride, size_t nframes, int holdTime, float decay, float intercept, float slope,
                         float *averages, float *peaks, int *holds) {
    maxiFFTOctaveAnalyzer *o = (maxiFFTOctaveAnalyzer *)h;
    o->peakHoldTime = holdTime;
    o->peakDecayRate = decay;
    o->linearEQIntercept = intercept;
    o->linearEQSlope = slope;
    const int nA = o->nAverages;
    for (size_t f = 0; f < nframes; f++) {
        o->calculate(mags + f * stride);
        memcpy(averages + f * nA, o->averages, sizeof(float) * nA);
        memcpy(peaks + f * nA, o->peaks, sizeof(float) * nA);
        memcpy(holds + f * nA, o->peakHoldTimes, sizeof(int) * nA);
    }
}

void bnd_ref_octave_free(void *h) { delete (maxiFFTOctaveAnalyzer *)h; }

}  // extern "C"
