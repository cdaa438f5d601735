// host/facade_atoms_smoke.cpp -- maxiAtomBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).  Checks what needs no
// reference: three streams with three books played in uneven blocks, raw atoms added by hand between two blocks, both onset modes,
// equal mxg_atoms_play_host / mxg_atoms_fill_host (the same arithmetic on the CPU) on the same blocks BIT FOR BIT; a bank without
// atoms leaves the block as it was; a raw atom outside the pool and a queue past its capacity are refused.
// Exit status 0 = all of it held.
//
//   facade_atoms_smoke
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                       \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "facade_atoms_smoke: %s failed\n", #c);     \
            fails++;                                                    \
        }                                                               \
    } while (0)

int main() {
    try {
        const size_t S = 3, Q = 8;
        typedef maxiAtomBank::BookAtom BA;
        const std::vector<std::vector<BA>> books = {{{0, 63, 20, 0.02f, 0}, {64, 257, 12, 0.3f, 1}, {128, 2, 30, 0.9f, -1}},
                                                    {{0, 65, 30, 0.07f, 0.2f}, {128, 64, 22, 0.4f, 0}},
                                                    {}};
        const std::vector<uint32_t> ns = {256, 192, 64};
        std::vector<float> raw(50);
        for (size_t i = 0; i < raw.size(); i++) raw[i] = 0.02f * (float)i - 0.5f;
        for (int onset = 0; onset < 2; onset++) {
            maxiAtomBank bank(S, Q, books, ns, raw);
            // the host twin: the same bank in host memory
            std::vector<int64_t> start = {0, 3, 5, 5};
            std::vector<float> rows(25);
            for (size_t s = 0, k = 0; s < S; s++)
                for (const BA &a : books[s]) {
                    rows[k] = a.position, rows[5 + k] = a.length, rows[10 + k] = a.amp, rows[15 + k] = a.frequency, rows[20 + k] = a.phase;
                    k++;
                }
            mxg_atoms_bank *host = mxg_atoms_bank_create_host(S, Q, start.data(), rows.data(), ns.data(), raw.data(), raw.size());
            EXPECT(host != nullptr);
            const size_t blocks[] = {64, 64, 7, 57, 64, 1, 63, 64};
            int blk = 0;
            for (size_t N : blocks) {
                if (blk == 2) {
                    bank.addAtom(2, 0, 50, 3);
                    bank.addAtom(0, 10, 40);
                    const int32_t st[2] = {2, 0}, kind[2] = {MXG_ATOM_RAW, MXG_ATOM_RAW};
                    const uint32_t len[2] = {50, 40}, off[2] = {3, 0}, at[2] = {0, 10};
                    EXPECT(mxg_atoms_add_host(host, 2, st, kind, len, off, nullptr, at) == 0);
                }
                std::vector<float> init(S * N), exp(S * N);
                for (size_t i = 0; i < init.size(); i++) init[i] = 0.001f * (float)(i % 17);
                exp = init;
                DeviceArray<float> d(S * N);
                d.upload(init);
                const bool play = blk != 5;
                if (play) bank.play(N, d.get(), onset);
                else bank.fillNextBuffer(N, d.get(), onset);
                EXPECT((play ? mxg_atoms_play_host(host, N, exp.data(), onset, 1) : mxg_atoms_fill_host(host, N, exp.data(), onset, 1)) == 0);
                maxigpu::check(mxg_sync(), "mxg_sync");
                const std::vector<float> got = d.download();
                EXPECT(got.size() == exp.size() && !memcmp(got.data(), exp.data(), exp.size() * sizeof(float)));
                if (blk == 0) EXPECT(memcmp(got.data(), init.data(), N * sizeof(float)) != 0 && !memcmp(got.data() + 2 * N, init.data() + 2 * N, N * sizeof(float)));
                blk++;
            }
            std::vector<int64_t> hidx(S);
            EXPECT(mxg_atoms_state(host, hidx.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0 && bank.sampleIdx() == hidx && hidx[0] == 384);
            mxg_atoms_bank_destroy(host);
        }
        maxiAtomBank small(1, 2, {}, {}, raw);
        bool refused = false;
        try { small.addAtom(0, 20, 31); } catch (const std::exception &) { refused = true; }
        EXPECT(refused);  // floats [20, 51) of a pool of 50
        small.addAtom(0, 0, 5);
        small.addAtom(0, 0, 5);
        refused = false;
        try { small.addAtom(0, 0, 5); } catch (const std::exception &) { refused = true; }
        EXPECT(refused && small.liveCount()[0] == 2);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_atoms_smoke: %s\n", e.what());
        return 1;
    }
    if (!fails) printf("facade_atoms_smoke: ok\n");
    return fails ? 1 : 0;
}
