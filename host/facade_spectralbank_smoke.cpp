// host/facade_spectralbank_smoke.cpp -- maxiFFTBank / maxiIFFTBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// A sine per voice: the first frame's peak bin is where the voice's frequency puts it.  Then ffttest.cpp's chain over V voices --
// maxiFFTBank -> maxiIFFTBank in after-FFT mode -- in one call and in an unaligned split: the same bits, and a signal comes out.
// Exit status 0 = all of it held.
//
//   facade_spectralbank_smoke
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                              \
    do {                                                                       \
        if (!(c)) {                                                            \
            fprintf(stderr, "facade_spectralbank_smoke: %s failed\n", #c);     \
            fails++;                                                           \
        }                                                                      \
    } while (0)

int main() {
    try {
        maxigpu::check(mxg_settings(44100, 2, 512), "mxg_settings");
        const size_t V = 70, N = 2048;
        const int fs = 1024, hop = 256, bins = fs / 2;
        std::vector<double> x(N * V);
        std::vector<int> bin_of(V);
        for (size_t v = 0; v < V; v++) {
            bin_of[v] = 8 + 5 * (int)v;  // a whole number of cycles per fftSize: the peak is that bin
            for (size_t n = 0; n < N; n++) x[n * V + v] = 0.5 * sin(2.0 * M_PI * (double)bin_of[v] * (double)n / (double)fs);
        }
        DeviceArray<double> dx(N * V), dy(N * V), dy2(N * V);
        dx.upload(x);

        // one call
        maxiFFTBank fa(V, fs, hop);
        maxiIFFTBank ia(V, fs, hop);
        const size_t F = fa.frames(N);
        EXPECT(F == N / hop && ia.rows(N, maxiIFFTBank::AFTER_FFT) == F && ia.rows(N) == N / hop);
        DeviceArray<float> mags(V * F * bins), phases(V * F * bins);
        fa.process(dx.get(), N, mags.get(), phases.get());
        ia.process(mags.get(), phases.get(), N, dy.get(), maxiIFFTBank::SPECTRUM, maxiIFFTBank::AFTER_FFT);
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<float> hm = mags.download();
        // frame 3 is the first that holds fftSize samples of the sine (frames 0..2 start inside the zeros of setup)
        size_t right = 0;
        for (size_t v = 0; v < V; v++) {
            const float *row = &hm[(3 * V + v) * bins];
            int peak = 0;
            for (int b = 1; b < bins; b++)
                if (row[b] > row[peak]) peak = b;
            right += peak == bin_of[v];
        }
        printf("first full frame: peak bin of voice 0 = %d, of voice %zu = %d; %zu of %zu voices on their bin\n", bin_of[0], V - 1,
               bin_of[V - 1], right, V);
        EXPECT(right == V);

        // the same in an unaligned split
        maxiFFTBank fb(V, fs, hop);
        maxiIFFTBank ib(V, fs, hop);
        const size_t parts[4] = {100, 411, 1, N - 512};
        size_t done = 0;
        for (size_t p = 0; p < 4; p++) {
            const size_t n = parts[p], f = fb.frames(n);
            EXPECT(ib.rows(n, maxiIFFTBank::AFTER_FFT) == f);
            DeviceArray<float> m(V * f * bins + 1), ph(V * f * bins + 1);
            fb.process(dx.get() + done * V, n, m.get(), ph.get());
            ib.process(m.get(), ph.get(), n, dy2.get() + done * V, maxiIFFTBank::SPECTRUM, maxiIFFTBank::AFTER_FFT);
            maxigpu::check(mxg_sync(), "mxg_sync");
            done += n;
        }
        EXPECT(done == N && fb.pos() == fa.pos() && ib.pos() == ia.pos());
        const std::vector<double> y = dy.download(), y2 = dy2.download();
        EXPECT(memcmp(y.data(), y2.data(), N * V * sizeof(double)) == 0);
        double sq = 0;
        size_t nan = 0;
        for (size_t i = (N / 2) * V; i < N * V; i++) {
            sq += y[i] * y[i];
            nan += y[i] != y[i];
        }
        const double rms = sqrt(sq / (double)((N / 2) * V));
        printf("chain output RMS over the second half = %.6f\n", rms);
        EXPECT(nan == 0);
        EXPECT(rms > 0.05 && rms < 1.0);  // Hann analysis x Hann synthesis at hop = fftSize / 4: gain 3/4 on 0.5 / sqrt(2)
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_spectralbank_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_spectralbank_smoke OK\n");
    return 0;
}
