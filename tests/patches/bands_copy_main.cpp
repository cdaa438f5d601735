// tests/patches/bands_copy_main.cpp -- stand-alone program (tests/test_gpu_bands_dropin.py): the drop-in maxiBark and
// maxiFFTOctaveAnalyzer are value types.  Both run a few frames, are copied mid-stream (copy construction, and assignment over an
// object set up differently), and copy and original continue over the same frames: every output, the public arrays and the
// parameters must stay identical, bit for bit.  An analyser assigned from one that was never set up is one.  Exit status 0 = held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian.h"
#include "maxiBark.h"

static int fails = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "bands_copy_main: %s failed\n", #c);      \
            fails++;                                                  \
        }                                                             \
    } while (0)

static std::vector<float> frame(int k) {  // bursts that decay: peaks rise, hold, count down and decay
    std::vector<float> x(512);
    const float level = (k % 5 == 0) ? 1.0f : 1.0f / (float)(1 + (k % 5) * 2);
    for (int i = 0; i < 512; i++) x[i] = level * (float)(((i * 37 + k * 101) % 97) + 1) / 97.0f;
    return x;
}

static bool same_oct(maxiFFTOctaveAnalyzer &a, maxiFFTOctaveAnalyzer &b) {
    return a.nAverages == b.nAverages && a.nSpectrum == b.nSpectrum && a.nAveragesPerOctave == b.nAveragesPerOctave &&
           a.samplingRate == b.samplingRate && a.spectrumFrequencySpan == b.spectrumFrequencySpan &&
           a.firstOctaveFrequency == b.firstOctaveFrequency && a.averageFrequencyIncrement == b.averageFrequencyIncrement &&
           a.peakHoldTime == b.peakHoldTime && a.peakDecayRate == b.peakDecayRate && a.linearEQSlope == b.linearEQSlope &&
           a.linearEQIntercept == b.linearEQIntercept && a.averages != b.averages && a.peaks != b.peaks && a.spe2avg != b.spe2avg &&
           !memcmp(a.averages, b.averages, sizeof(float) * a.nAverages) && !memcmp(a.peaks, b.peaks, sizeof(float) * a.nAverages) &&
           !memcmp(a.peakHoldTimes, b.peakHoldTimes, sizeof(int) * a.nAverages) && !memcmp(a.spe2avg, b.spe2avg, sizeof(int) * a.nSpectrum);
}

int main() {
    maxiBark bark;
    bark.setup(44100, 1024);
    maxiFFTOctaveAnalyzer oct1;
    oct1.setup(44100, 512, 12);
    oct1.peakHoldTime = 2;
    oct1.peakDecayRate = 0.8f;
    oct1.linearEQSlope = 0.003f;
    oct1.linearEQIntercept = 0.5f;
    maxiFFTOctaveAnalyzer assigned;
    assigned.setup(22050, 256, 3);  // set up differently, then assigned over
    maxiBark bark_assigned;
    bark_assigned.setup(8000, 64);
    for (int k = 0; k < 6; k++) {
        std::vector<float> x = frame(k);
        bark.relativeLoudness(x.data());
        bark.totalLoudness(x.data());
        oct1.calculate(x.data());
    }
    bool held = false, nonzero = false;
    for (int i = 0; i < oct1.nAverages; i++) {
        held = held || oct1.peakHoldTimes[i] > 0 || oct1.peaks[i] > oct1.averages[i];
        nonzero = nonzero || oct1.averages[i] != 0.0f;
    }
    EXPECT(held && nonzero);  // the copy is taken mid-stream: a peak is above its average
    maxiBark bark_copy(bark);
    bark_assigned = bark;
    maxiFFTOctaveAnalyzer copy(oct1);
    assigned = oct1;
    EXPECT(same_oct(oct1, copy) && same_oct(oct1, assigned));
    EXPECT(copy.peakHoldTime == 2 && copy.peakDecayRate == 0.8f && copy.linearEQSlope == 0.003f && copy.linearEQIntercept == 0.5f);
    EXPECT(bark_copy.NUM_BARK_BANDS == 24);
    for (int k = 6; k < 16; k++) {
        std::vector<float> x = frame(k);
        double a[3][24], t[3];
        maxiBark *bs[3] = {&bark, &bark_copy, &bark_assigned};
        for (int i = 0; i < 3; i++) {
            memcpy(a[i], k % 2 ? bs[i]->specificLoudness(x.data()) : bs[i]->relativeLoudness(x.data()), sizeof(a[i]));
            t[i] = bs[i]->totalLoudness(x.data())[0];
        }
        EXPECT(!memcmp(a[0], a[1], sizeof(a[0])) && !memcmp(a[0], a[2], sizeof(a[0])) && t[0] == t[1] && t[0] == t[2] && t[0] > 0);
        if (k == 10) copy.peaks[3] = oct1.peaks[3] = assigned.peaks[3] = 100.0f;  // the public arrays are the state
        oct1.calculate(x.data());
        copy.calculate(x.data());
        assigned.calculate(x.data());
        EXPECT(same_oct(oct1, copy) && same_oct(oct1, assigned));
        if (k == 10) EXPECT(oct1.peaks[3] == 100.0f * 0.8f || oct1.peakHoldTimes[3] >= 0);
    }
    maxiFFTOctaveAnalyzer never;
    assigned = never;
    EXPECT(assigned.nAverages == 0 && assigned.nSpectrum == 0 && assigned.averages == nullptr && assigned.peaks == nullptr &&
           assigned.peakHoldTimes == nullptr && assigned.spe2avg == nullptr);
    maxiFFTOctaveAnalyzer empty_copy(never);
    EXPECT(empty_copy.nAverages == 0 && empty_copy.averages == nullptr);
    if (fails) return 1;
    printf("bands_copy_main: ok (peaks[3] %.9g, hold %d)\n", oct1.peaks[3], oct1.peakHoldTimes[3]);
    return 0;
}
