// host/facade_convolve_smoke.cpp -- maxiConvolveBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference: a block rendered in three calls equals the same block rendered in one (the rings and the pending
// sums are carried), play_nv() on doubles [N][V] equals play() on the narrowed, transposed block, every stream equals a
// maxiConvolveBlock of its own fed the same input, streams on an impulse shorter than one frame and the reference's mode are silent.
// Exit status 0 = all of it held.
//
//   facade_convolve_smoke
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            fprintf(stderr, "facade_convolve_smoke: %s failed\n", #c);     \
            fails++;                                                       \
        }                                                                  \
    } while (0)

int main() {
    try {
        maxigpu::check(mxg_settings(44100, 2, 512), "mxg_settings");
        const size_t V = 70, F = 64, nb = 21, N = nb * F;  // 21 blocks: two launches of the multiply-accumulate kernel, a ragged tile
        std::vector<std::vector<double>> imp(3);
        imp[0].resize(300);  // 5 frames
        imp[1].resize(20);   // shorter than one frame: no frame at all
        imp[2].resize(1000); // 16 frames
        for (size_t i = 0; i < imp.size(); i++)
            for (size_t s = 0; s < imp[i].size(); s++)
                imp[i][s] = (double)((s * (13 + 4 * i)) % 97) / 97.0 * (1.0 - (double)s / (double)imp[i].size()) - 0.2;
        std::vector<int> imp_of(V);
        for (size_t v = 0; v < V; v++) imp_of[v] = (int)(v % 3);
        std::vector<float> x(V * N);
        std::vector<double> xnv(N * V);
        for (size_t v = 0; v < V; v++)
            for (size_t n = 0; n < N; n++) {
                const double s = (double)((n * (7 + v % 5)) % 200) / 100.0 - 1.0 + 1e-9 * (double)v;  // (a part below float precision: play_nv narrows it away)
                xnv[n * V + v] = s;
                x[v * N + n] = (float)s;
            }
        DeviceArray<float> dx(V * N), one(V * N), ref0(V * N);
        DeviceArray<double> dnv(N * V), onv(N * V);
        dx.upload(x);
        dnv.upload(xnv);

        maxiConvolveBank a(V, imp, imp_of, (int)F, 16), b(V, imp, imp_of, (int)F, 16), c(V, imp, imp_of, (int)F, 16);
        EXPECT(a.frames(0) == 5 && a.frames(1) == 0 && a.frames(2) == 16);
        a.play(dx.get(), nb, one.get(), true);
        // three calls: [V][N] is stream-major, so a part of every stream's block is a strided view -- render the parts through buffers
        const size_t parts[3] = {2, 18, 1};
        size_t done = 0;
        std::vector<float> got(V * N);
        for (size_t p = 0; p < 3; p++) {
            const size_t n = parts[p] * F;
            std::vector<float> px(V * n);
            for (size_t v = 0; v < V; v++) memcpy(&px[v * n], &x[v * N + done * F], n * sizeof(float));
            DeviceArray<float> dpx(V * n), dpo(V * n);
            dpx.upload(px);
            b.play(dpx.get(), parts[p], dpo.get(), true);
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<float> po = dpo.download();
            for (size_t v = 0; v < V; v++) memcpy(&got[v * N + done * F], &po[v * n], n * sizeof(float));
            done += parts[p];
        }
        c.play_nv(dnv.get(), nb, onv.get(), true);
        a.reset();
        a.play(dx.get(), nb, ref0.get(), false);  // as the reference computes: silence
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<float> h1 = one.download(), h0 = ref0.download();
        const std::vector<double> hnv = onv.download();
        size_t same = 0, same_nv = 0, silent1 = 0, silent0 = 0, loud = 0, nan = 0;
        for (size_t v = 0; v < V; v++)
            for (size_t n = 0; n < N; n++) {
                const float o = h1[v * N + n];
                same += memcmp(&o, &got[v * N + n], sizeof(float)) == 0;
                same_nv += (double)o == hnv[n * V + v];
                nan += o != o;
                if (imp_of[v] == 1) silent1 += o == 0.0f;
                else loud += o != 0.0f;
                silent0 += h0[v * N + n] == 0.0f;
            }
        EXPECT(same == V * N);
        EXPECT(same_nv == V * N);
        EXPECT(nan == 0);
        EXPECT(silent1 == ((V + 1) / 3) * N);  // streams 1, 4, 7 ...: an impulse without a frame
        EXPECT(loud > V * N / 16);  // (maxiIFFT's window covers hopsize = 16 of a block's 64 samples: the rest is 0 in every stream)
        EXPECT(silent0 == V * N);

        // stream 2 (impulse 2) against a maxiConvolveBlock of its own
        maxiConvolveBlock single;
        single.setup(imp[2], (double)imp[2].size(), (int)F, 16);
        EXPECT(single.frames() == 16);
        DeviceArray<float> sx(N), so(N);
        sx.upload(&x[2 * N], N);
        single.play(sx.get(), nb, so.get(), true);
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<float> hs = so.download();
        EXPECT(memcmp(hs.data(), &h1[2 * N], N * sizeof(float)) == 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_convolve_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_convolve_smoke OK\n");
    return 0;
}
