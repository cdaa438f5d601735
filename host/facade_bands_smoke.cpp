// host/facade_bands_smoke.cpp -- maxiBarkBatch and maxiOctaveBatch of include/maximilian_bank.hpp from plain C++ (no HIP headers):
// maxiFFTBatch -> magnitudes -> both banks.  Checks what needs no reference, against values computed here with plain loops over
// the downloaded magnitudes: the Bark band sums (a double accumulated bin after bin between the plan's limits) to the bit,
// specific within 16 ULP of the host pow, relative exactly 1 at a frame's maximum, total within 39 * 2^-52; the octave averages,
// peaks and their carry over two calls to the bit.  Prints a few values.  Exit status 0 = all of it held.
//
//   facade_bands_smoke
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                       \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "facade_bands_smoke: %s failed\n", #c);     \
            fails++;                                                    \
        }                                                               \
    } while (0)

static double ulps(double a, double b) {  // distance in ULPs of b
    if (a == b) return 0;
    int e;
    frexp(b, &e);
    return fabs(a - b) / ldexp(1.0, e - 53);
}

int main() {
    try {
        maxiSettings::setup(44100, 2, 1024);
        const size_t S = 3, K = 7, F = S * K, B = 512, hop = 200;
        std::vector<float> sig((F - 1) * hop + 1024);
        for (size_t i = 0; i < sig.size(); i++)
            sig[i] = (float)(0.6 * sin(0.031 * (double)i) + 0.3 * sin(0.71 * (double)i) * (1.0 + sin(0.0009 * (double)i)));
        DeviceArray<float> d_sig(sig.size()), d_mags(F * B);
        d_sig.upload(sig);
        maxiFFTBatch fft;
        fft.setup(1024, 512, 1024);
        fft.process(d_sig.get(), hop, F, d_mags.get(), nullptr);
        const std::vector<float> mags = d_mags.download();

        // ---- maxiBark ------------------------------------------------------------------------------------------------------
        maxiBarkBatch bark;
        bark.setup(44100, 1024);
        const std::vector<int> lim = bark.limits();
        EXPECT(lim.size() == 25 && lim[0] == 0 && lim[24] == 511);
        DeviceArray<double> d_sum(F * 24), d_spec(F * 24), d_rel(F * 24), d_tot(F);
        bark.analyse(d_mags.get(), F, d_spec.get(), d_rel.get(), d_tot.get(), d_sum.get());
        const std::vector<double> sum = d_sum.download(), spec = d_spec.download(), rel = d_rel.download(), tot = d_tot.download();
        double worst = 0;
        for (size_t f = 0; f < F; f++) {
            double mx = 0, total = 0;
            for (int b = 0; b < 24; b++) {
                double s = 0;
                for (int j = lim[b]; j < lim[b + 1]; j++) s += mags[f * B + j];
                EXPECT(!memcmp(&s, &sum[f * 24 + b], sizeof(double)));
                const double sp = pow(s, 0.23);
                const double u = ulps(spec[f * 24 + b], sp);
                worst = u > worst ? u : worst;
                if (spec[f * 24 + b] > mx) mx = spec[f * 24 + b];
                total += sp;
            }
            EXPECT(fabs(tot[f] - total) <= 39 * ldexp(1.0, -52) * total);
            double rmax = 0;
            for (int b = 0; b < 24; b++) {
                rmax = rel[f * 24 + b] > rmax ? rel[f * 24 + b] : rmax;
                EXPECT(rel[f * 24 + b] == spec[f * 24 + b] / mx);
            }
            EXPECT(rmax == 1.0);
        }
        EXPECT(worst <= 16);
        printf("bark: limits 1 / 12 / 23 = %d %d %d, frame 0 specific[3] %.17g relative[3] %.17g total %.17g, worst %g ULP\n", lim[1], lim[12],
               lim[23], spec[3], rel[3], tot[0], worst);

        // ---- maxiFFTOctaveAnalyzer: S analysers over K frames each, twice over the same rows, state carried ----
        maxiOctaveBatch oct(S);
        oct.setup(44100.0f, (int)B, 12);
        oct.peakHoldTime = 2;
        oct.linearEQSlope = 0.002f;
        const int nA = oct.nAverages();
        EXPECT(nA == 104);
        // the map, restated in float as the reference forms it
        std::vector<int> map(B);
        {
            const float span = (44100.0f / 2.0f) / (float)B, inc = powf(2.0f, 1.0f / 12.0f);
            float top = 55.0f, fr = span;
            int a = 0;
            for (size_t i = 0; i < B; i++) {
                while (fr > top) { a++; top *= inc; }
                map[i] = a;
                fr += span;
            }
            EXPECT(a == nA);
        }
        DeviceArray<float> d_avg(F * nA), d_pk(F * nA);
        std::vector<float> peak(S * nA, 0.0f);
        std::vector<int> hold(S * nA, 0);
        for (int call = 0; call < 2; call++) {
            oct.calculate(d_mags.get(), K, d_avg.get(), d_pk.get());
            const std::vector<float> avg = d_avg.download(), pk = d_pk.download();
            for (size_t s = 0; s < S; s++)
                for (size_t k = 0; k < K; k++) {
                    const size_t g = s * K + k;
                    std::vector<float> want(nA, 0.0f);
                    float acc = 0.0f;
                    int count = 0, last = 0;
                    for (size_t i = 0; i < B; i++) {
                        count++;
                        acc += mags[g * B + i] * (oct.linearEQIntercept + (float)i * oct.linearEQSlope);
                        if (map[i] != last) {
                            for (int j = last; j < map[i]; j++) want[j] = acc / (float)count;
                            count = 0;
                            acc = 0.0f;
                        }
                        last = map[i];
                    }
                    EXPECT(!memcmp(want.data(), &avg[g * nA], sizeof(float) * nA));
                    for (int a = 0; a < nA; a++) {
                        float &p = peak[s * nA + a];
                        int &h = hold[s * nA + a];
                        if (want[a] >= p) { p = want[a]; h = oct.peakHoldTime; }
                        else if (h > 0) h--;
                        else p *= oct.peakDecayRate;
                    }
                    EXPECT(!memcmp(&peak[s * nA], &pk[g * nA], sizeof(float) * nA));
                }
            if (call == 1) printf("octave: %d averages, last frame averages[40] %.9g peaks[40] %.9g\n", nA, avg[(F - 1) * nA + 40], pk[(F - 1) * nA + 40]);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_bands_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_bands_smoke: ok\n");
    return 0;
}
