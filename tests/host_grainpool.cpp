// tests/host_grainpool.cpp -- TEST INFRASTRUCTURE.  The host build of maximilian_amd/csrc/mxg_grainpool.h (K27's arithmetic) behind a
// C interface for tests/grainpool_host.py, compiled by g++ under the oracle's FPFLAGS.  With -DGPOOL_HOST_MAIN it is a stand-alone
// program (for the sanitizers: AddressSanitizer + UndefinedBehaviorSanitizer) that replays a file of recorded calls -- the whole
// golden table, call by call, as tests/test_grainpool_host.py records it -- with every slot's tail and the gaps between the slots
// poisoned, so that a read outside [0, len) of a stream's slot is an error and not a silent zero.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mxg_grainpool.h"

using namespace mxg;

static int g_tiles = 0;

extern "C" {

int gp_h_render(int mode, size_t S, size_t T, const double *pool, size_t stride, size_t cap, size_t R, const uint64_t *len, const uint32_t *slot,
                const uint64_t *loop, const double *window, int sampleDur, double grainLength, double sr, int overlaps, const double *a,
                const double *b, const double *posmod, int ps, const int32_t *rnd, size_t Rn, double *st, double *gst, double *out) {
    GpArgs A;
    A.S = S; A.T = T; A.R = R; A.stride = stride; A.cap = cap; A.Rn = Rn;
    A.pool = pool; A.len = len; A.slot = slot; A.loop = loop; A.window = window;
    A.a = a; A.b = b; A.posMod = posmod; A.ps = ps; A.rnd = rnd;
    A.st = st; A.gst = gst; A.out = out;
    A.sr = sr;
    A.cycleLength = grainLength * sr / overlaps;
    A.grainLength = grainLength;
    A.sampleDur = sampleDur;
    if (!g_tiles) return gp_host_render(mode, A);
    // the tile form: the scheduler pass, then every sample on its own, as K27's render pass cuts the call
    GpLists L;
    L.G = gp_lists_births(T, A.cycleLength);
    L.C = (T + kGpTile - 1) / kGpTile;
    std::vector<int32_t> bn(L.G * S), first((L.C + 1) * S);
    std::vector<double> bp(L.G * S), bi(L.G * S), gin(4 * kGpSlots * S);
    L.birth_n = bn.data(); L.birth_pos = bp.data(); L.birth_inc = bi.data(); L.first = first.data(); L.gst_in = gin.data();
    return gp_host_render_tiles(mode, A, L);
}

void gp_h_tiles(int on) { g_tiles = on; }

// gp_advance (the exact multi-step forms) and the recurrence it stands for, step by step
double gp_h_advance(double pos, double inc, double dlen, int steps) { return gp_advance(pos, inc, dlen, steps); }
double gp_h_advance_plain(double pos, double inc, double dlen, int steps) {
    for (int i = 0; i < steps; i++) {
        pos = pos + inc;
        if (pos >= dlen)
            pos -= dlen;
        else if (pos < 0)
            pos += dlen;
    }
    return pos;
}

const char *gp_h_loop(uint64_t len, double start01, double end01, uint64_t *loopStart, uint64_t *loopEnd) {
    return gp_stretch_loop(len, start01, end01, loopStart, loopEnd);
}

}  // extern "C"

#ifdef GPOOL_HOST_MAIN
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define GP_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define GP_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define GP_POISON(p, n) ((void)0)
#define GP_UNPOISON(p, n) ((void)0)
#endif

template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// file: int64 [R, stride, cap, guard], uint64 len[R], double mem[guard + R * stride]; then per call int64 hdr[12] = mode, S, n,
// overlaps, ps, Rn, window length, count of a, of b, of posMod, has loop, has rnd; then window, slot u32 [S], loop u64 [2][S], a, b,
// posMod, rnd i32 [S][Rn], st [4][S], gst [4][8][S].
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> h;
    std::vector<uint64_t> len;
    std::vector<double> mem;
    if (!rd(f, h, 4)) return 3;
    const size_t R = (size_t)h[0], stride = (size_t)h[1], cap = (size_t)h[2], guard = (size_t)h[3];
    if (!rd(f, len, R) || !rd(f, mem, guard + R * stride)) return 3;
    GP_POISON(mem.data(), guard * sizeof(double));
    for (size_t r = 0; r < R; r++) GP_POISON(mem.data() + guard + r * stride + len[r], (stride - len[r]) * sizeof(double));
    int calls = 0, failed = 0;
    double acc = 0.0;
    while (rd(f, h, 12)) {
        const int mode = (int)h[0];
        const size_t S = (size_t)h[1], n = (size_t)h[2], Rn = (size_t)h[5];
        std::vector<double> win, a, b, pm, st, gst, out(n * S);
        std::vector<uint32_t> slot;
        std::vector<uint64_t> loop;
        std::vector<int32_t> rnd;
        if (!rd(f, win, (size_t)h[6]) || !rd(f, slot, S) || !rd(f, loop, h[10] ? 2 * S : 0) || !rd(f, a, (size_t)h[7]) || !rd(f, b, (size_t)h[8]) ||
            !rd(f, pm, (size_t)h[9]) || !rd(f, rnd, h[11] ? S * Rn : 0) || !rd(f, st, 4 * S) || !rd(f, gst, 32 * S))
            return 3;
        failed |= gp_h_render(mode, S, n, mem.data() + guard, stride, cap, R, len.data(), slot.data(), h[10] ? loop.data() : nullptr, win.data(),
                              (int)win.size(), 0.01, 44100.0, (int)h[3], a.data(), h[8] ? b.data() : nullptr, h[9] ? pm.data() : nullptr, (int)h[4],
                              h[11] ? rnd.data() : nullptr, Rn, st.data(), gst.data(), out.data());
        for (double v : out) acc += v;
        calls++;
    }
    fclose(f);
    GP_UNPOISON(mem.data(), mem.size() * sizeof(double));
    // the refusals of the loop conversion
    uint64_t ls = 0, le = 0;
    const double nan = __builtin_nan("");
    int refused = 0;
    refused += gp_h_loop(4096, nan, 0.5, &ls, &le) != nullptr;
    refused += gp_h_loop(4096, -0.25, 0.5, &ls, &le) != nullptr;
    refused += gp_h_loop(4096, 0.5, 0.5, &ls, &le) != nullptr;
    refused += gp_h_loop(4096, 0.5, 1.5, &ls, &le) != nullptr;
    refused += gp_h_loop(4096, 0.5, 1e300, &ls, &le) != nullptr;
    refused += gp_h_loop(4096, 0.25, 0.5, &ls, &le) == nullptr && ls == 1024 && le == 2048;
    printf("host_grainpool: ok calls=%d failed=%d refused=%d (%g)\n", calls, failed, refused, acc);
    return (failed == 0 && refused == 6 && calls > 0) ? 0 : 1;
}
#endif
