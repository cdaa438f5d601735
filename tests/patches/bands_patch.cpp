// tests/patches/bands_patch.cpp -- a patch written against the reference's API: an arithmetic signal -> maxiFFT(1024, 512) -> on
// each new frame maxiBark::specificLoudness and maxiFFTOctaveAnalyzer::calculate over the magnitudes (not magnitudesDB, whose
// log10f would turn the octave channel into a tolerance test).  Channel 0 cycles through averages / peaks, channel 1 through the
// specific loudness.  It touches every public member of maxiFFTOctaveAnalyzer and maxiBark::NUM_BARK_BANDS.
#include "maximilian.h"
#include "libs/maxim.h"

maxiFFT fft;
maxiBark bark;
maxiFFTOctaveAnalyzer octv;
static int n = 0, slot = 0;
static double *specific = nullptr;

void setup() {
    fft.setup(1024, 512, 1024);
    bark.setup(44100, 1024);
    octv.setup(44100, 512, 12);
    octv.peakHoldTime = 2;
    octv.peakDecayRate = 0.9f;
    octv.linearEQIntercept = 1.0f;
    octv.linearEQSlope = 0.002f;
    for (int i = 0; i < octv.nAverages; i++) {  // (the reference leaves them uninitialised)
        octv.averages[i] = 0.0f;
        octv.peaks[i] = 0.0f;
        octv.peakHoldTimes[i] = 0;
    }
}

void play(double *output) {
    const int k = n++;
    const float x = (float)(((k * 7919) % 2001 - 1000) / 1000.0) * (float)(0.25 + 0.75 * ((k / 700) % 5 == 0));
    if (fft.process(x)) {
        specific = bark.specificLoudness(&fft.getMagnitudes()[0]);
        octv.calculate(&fft.getMagnitudes()[0]);
        slot = 0;
    }
    const int nA = octv.nAverages > 0 ? octv.nAverages : 1;
    const int j = slot % nA;
    output[0] = (slot / nA) % 2 == 0 ? (double)octv.averages[j] : (double)octv.peaks[j] + 0.001 * octv.peakHoldTimes[j];
    output[1] = specific ? specific[slot % bark.NUM_BARK_BANDS] : 0.0;
    output[1] += 0.0 * (octv.samplingRate + octv.nSpectrum + octv.nAveragesPerOctave + octv.spectrumFrequencySpan + octv.firstOctaveFrequency +
                        octv.averageFrequencyIncrement + octv.spe2avg[0] + octv.peakHoldTime + octv.peakDecayRate + octv.linearEQSlope +
                        octv.linearEQIntercept);
    slot++;
}
