// tests/host_bands.cpp -- host build of mxg_bands.h (tests/test_bands_host.py).  The bnd_host_* functions take the arguments of
// mxg_bark_batch / mxg_octave_batch (include/maxigpu.h) without plan and stream, on host arrays in the same layouts, and run the
// step functions the kernels of bands.hip run, frame after frame.  With -DBND_HOST_MAIN the file is a stand-alone program that
// plays both analysers over small shapes, empty bands, NaN / Inf / negative inputs and state carried over calls (the sanitizer run).
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "mxg_bands.h"

using namespace mxg;

extern "C" {

int bnd_host_bark_limits(unsigned sR, unsigned bS, int *lim) {
    if (bS < 2 || bS > MXG_BARK_MAX_BUFFER || (uint64_t)(bS / 2 - 1) * sR > 0xffffffffull) return -1;
    std::vector<double> scale(bS / 2);
    bnd_bark_limits(sR, bS, lim, scale.data());
    return 0;
}

int bnd_host_octave_map(float sr, int n, int perOctave, int *map) { return bnd_octave_map(sr, n, perOctave, map, nullptr, nullptr); }

int bnd_host_bark(const int *lim, const float *spec, size_t stride, size_t nframes, double *bandsum, double *specific, double *relative,
                  double *total) {
    for (size_t f = 0; f < nframes; f++) {
        double v[MXG_BARK_BANDS], mx, tot;
        for (int b = 0; b < MXG_BARK_BANDS; b++) v[b] = bnd_bark_band(spec + f * stride, lim[b], lim[b + 1]);
        if (bandsum)
            for (int b = 0; b < MXG_BARK_BANDS; b++) bandsum[f * MXG_BARK_BANDS + b] = v[b];
        bnd_bark_loudness(v, mx, tot);
        if (specific)
            for (int b = 0; b < MXG_BARK_BANDS; b++) specific[f * MXG_BARK_BANDS + b] = v[b];
        if (total) total[f] = tot;
        if (relative) {
            bnd_bark_relative(v, mx);
            for (int b = 0; b < MXG_BARK_BANDS; b++) relative[f * MXG_BARK_BANDS + b] = v[b];
        }
    }
    return 0;
}

int bnd_host_octave(const int *map, int nSpectrum, int nAverages, const float *mags, size_t stride, size_t nstreams, size_t fps,
                    float intercept, float slope, int holdTime, float decay, float *averages, float *peaks_out, float *peak_state,
                    int32_t *hold_state) {
    for (size_t s = 0; s < nstreams; s++)
        for (size_t k = 0; k < fps; k++) {
            const size_t g = s * fps + k;
            float *avg = averages + g * nAverages;
            bnd_octave_frame(mags + g * stride, nSpectrum, map, nAverages, intercept, slope, avg);
            if (!peak_state) continue;
            for (int a = 0; a < nAverages; a++) {
                bnd_peak_step(avg[a], peak_state[s * nAverages + a], hold_state[s * nAverages + a], holdTime, decay);
                if (peaks_out) peaks_out[g * nAverages + a] = peak_state[s * nAverages + a];
            }
        }
    return 0;
}

}  // extern "C"

#ifdef BND_HOST_MAIN
int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    double acc = 0;
    const unsigned rates[] = {44100, 22050, 8000, 96000, 0, 1000};
    for (unsigned sr : rates)
        for (unsigned bs : {2u, 3u, 16u, 64u, 1024u, 4096u}) {
            int lim[MXG_BARK_BANDS + 1];
            if (bnd_host_bark_limits(sr, bs, lim)) continue;
            const size_t spec = bs / 2, nf = 5;
            std::vector<float> x(nf * spec);  // exactly the rows: a read past a row's end is a report
            for (size_t i = 0; i < x.size(); i++) x[i] = (float)((i * 37) % 11) * 0.125f;
            for (size_t i = 0; i < spec; i++) x[spec + i] = 0.0f;
            x[2 * spec] = nan;
            x[3 * spec] = -4.0f;
            x[4 * spec + spec / 2] = inf;
            std::vector<double> a(nf * 24), b(nf * 24), c(nf * 24), t(nf);
            bnd_host_bark(lim, x.data(), spec, nf, a.data(), b.data(), c.data(), t.data());
            bnd_host_bark(lim, x.data(), spec, nf, nullptr, nullptr, nullptr, t.data());
            acc += t[0] + a[23] + lim[24];
        }
    for (float sr : {44100.0f, 8000.0f, 96000.0f, 200.0f})
        for (int n : {1, 8, 16, 512, 4096})
            for (int per : {0, 1, 3, 12, 24}) {
                std::vector<int> map(n);
                const int nA = bnd_host_octave_map(sr, n, per, map.data());
                if (nA <= 0) continue;
                const size_t S = 2, K = 3;
                std::vector<float> x(S * K * n), avg(S * K * nA), pk(S * K * nA), ps(S * nA, 0.0f);
                std::vector<int32_t> hs(S * nA, 0);
                for (size_t i = 0; i < x.size(); i++) x[i] = (float)((i * 13) % 7) - 1.0f;
                x[n / 2] = nan;
                for (int rep = 0; rep < 3; rep++)
                    bnd_host_octave(map.data(), n, nA, x.data(), n, S, K, 1.0f, 0.01f, rep, 0.9f, avg.data(), rep ? pk.data() : nullptr,
                                    ps.data(), hs.data());
                bnd_host_octave(map.data(), n, nA, x.data(), n, S, K, 1.0f, 0.0f, 0, 0.9f, avg.data(), nullptr, nullptr, nullptr);
                acc += avg[nA - 1] == avg[nA - 1] ? avg[nA - 1] : 0.0f;
                acc += hs[0];
            }
    printf("host_bands: ok (%g)\n", acc);
    return 0;
}
#endif
