// tests/host_atoms.cpp -- host build of mxg_atoms.h with g++: a stand-alone program (its own main) over the host forms of K22.
//   1. atoms_sin against quad precision (sinq) on float arguments up to 2^19 rad: a seeded sweep of the whole range, the two floats
//      next to every multiple of pi/2 in it (the arguments that come closest to a zero or an extremum of the function), small and tiny
//      arguments.  The error has to stay below 1 ULP of the double result, so that the float it rounds to is one of the two floats
//      bracketing the true value; the program prints the largest error and how often the rounded float is not the nearest one.
//   2. the queue: seeded scripts of addAtom / play / fill through atoms_stream_step and atoms_seg_render -- block lengths 1 to 600 that
//      change between calls (entries stall), both onset modes, Gabor and raw atoms, atoms of 0 and 1 samples, a live list at capacity
//      and one past it (the step returns -1 and changes nothing) -- with every segment checked against the block and the atom.
// Built with -fsanitize=address,undefined and run once on the CPU; tests/test_atoms_host.py builds it without the sanitizers and
// checks its verdict.
#include <quadmath.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mxg_atoms.h"

using namespace mxg;

static uint32_t lcg = 20221101u;
static uint32_t rnd() { return lcg = lcg * 1664525u + 1013904223u; }

static double worst = 0;
static size_t nargs = 0, not_nearest = 0;
static void sin_check(float xf) {
    const double x = xf, got = atoms_sin(x);
    const __float128 ref = sinq((__float128)x);
    const double refd = (double)ref;
    const double ulp = ldexp(1.0, ilogb(refd == 0 ? 1e-300 : refd) - 52);
    const double e = (double)fabsq(((__float128)got - ref) / (__float128)ulp);
    if (e > worst) worst = e;
    if ((float)got != (float)ref) not_nearest++;
    nargs++;
}

static int queue_check() {
    const size_t Q = 24;
    std::vector<float> win, raw(4096);
    for (auto &v : raw) v = (float)((int32_t)rnd() / 2147483648.0);
    const uint32_t lens[] = {1, 2, 63, 64, 65, 257};
    std::vector<uint32_t> woff;
    for (uint32_t len : lens) {
        woff.push_back((uint32_t)win.size());
        for (uint32_t i = 0; i < len; i++) win.push_back((float)gabor_window(len, i));
    }
    // a book of 12 atoms, positions multiples of 16, some out of order
    std::vector<float> pos;
    std::vector<AtomInst> inst;
    for (int k = 0; k < 12; k++) {
        const int li = k % 6;
        const GaborPar p = gabor_params(book_freq(0.08f * k), kBookSampleRate, lens[li]);
        pos.push_back((float)(16 * ((k * 5) % 12)));
        inst.push_back({0, 0, lens[li], MXG_ATOM_GABOR, woff[li], p.inc, p.maxPhase, 0.1f * k, book_amp(20.0f + k)});
    }
    double acc = 0;
    for (int onset = 0; onset < 2; onset++)
        for (int round = 0; round < 40; round++) {
            const AtomBookView book = {pos.data(), inst.data(), (uint32_t)(round % 3 ? 12 : 0), 192};
            int64_t sampleIdx = 0;
            uint32_t atomIdx = 0;
            int32_t nlive = 0;
            std::vector<AtomInst> live(Q);
            std::vector<AtomSeg> seg(Q);
            for (int blk = 0; blk < 30; blk++) {
                const uint32_t N = (blk % 4 == 3) ? 16 : 1 + rnd() % 600;
                for (int a = rnd() % 3; a > 0 && (size_t)nlive < Q; a--) {  // addAtom of a raw atom of 0 .. 300 samples
                    const uint32_t size = (rnd() % 5 == 0) ? rnd() % 2 : rnd() % 300, off = rnd() % 3000;
                    live[nlive++] = {sampleIdx + (int64_t)(rnd() % 40), 0, size, MXG_ATOM_RAW, off, 0.f, 0.f, 0.f, 0.f};
                }
                const std::vector<AtomInst> before(live.begin(), live.begin() + nlive);
                const int64_t idx0 = sampleIdx;
                const int n = atoms_stream_step(blk % 2 == 0, book, onset, N, Q, sampleIdx, atomIdx, nlive, live.data(), seg.data());
                if (n < 0) {  // overflow: nothing changed
                    if (sampleIdx != idx0 || (size_t)nlive != before.size() || memcmp(before.data(), live.data(), before.size() * sizeof(AtomInst))) return 1;
                    nlive = 0;
                    continue;
                }
                if (sampleIdx != idx0 + (int64_t)N || (size_t)n > Q || (size_t)nlive > Q) return 2;
                std::vector<float> buf(N, 0.25f);
                for (int k = 0; k < n; k++) {
                    const AtomSeg &g = seg[k];
                    if (!g.count || (size_t)g.dst_off + g.count > N || (onset == MXG_ATOM_ONSET_BLOCK && g.dst_off)) return 3;
                    if (g.kind == MXG_ATOM_RAW ? (size_t)g.off + g.src_pos + g.count > raw.size() : (size_t)g.off + g.src_pos + g.count > win.size()) return 4;
                    atoms_seg_render(g, win.data(), raw.data(), buf.data());
                }
                for (float v : buf) {
                    if (!(v == v)) return 5;
                    acc += v;
                }
                for (int k = 0; k < nlive; k++)
                    if (live[k].pos >= live[k].size) return 6;
            }
        }
    printf("host_atoms: queue ok (%g)\n", acc);
    return 0;
}

int main() {
    const double pio2 = 1.57079632679489661923;
    for (int i = 0; i < 2000000; i++) {  // the whole range, signs and magnitudes drawn evenly over the exponents 2^-20 .. 2^19
        const int e = (int)(rnd() % 40) - 20;
        const float m = 1.0f + (float)(rnd() >> 9) / 8388608.0f;
        sin_check(((rnd() & 1) ? -1.0f : 1.0f) * ldexpf(m, e));
    }
    for (int k = 1; k < 333772; k++) {  // the floats next to k pi / 2 < 2^19
        const float f = (float)(k * pio2);
        sin_check(f);
        sin_check(nextafterf(f, 0.0f));
        sin_check(nextafterf(f, 1e30f));
        sin_check(-f);
    }
    for (float f : {0.0f, -0.0f, 1e-30f, 1e-44f, 524288.0f, -524288.0f, 0.78539816f, 0.78539819f}) sin_check(f);
    printf("host_atoms: atoms_sin max error %.4f ULP over %zu float arguments; the rounded float is not the nearest on %zu\n", worst, nargs, not_nearest);
    if (!(worst < 1.0)) return 10;
    const int q = queue_check();
    if (q) {
        printf("host_atoms: queue check %d failed\n", q);
        return q;
    }
    printf("host_atoms: ok\n");
    return 0;
}
