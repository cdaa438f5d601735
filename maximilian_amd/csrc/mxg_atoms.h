// mxg_atoms.h -- the reference's Gabor atoms and its atom queue (src/libs/maxiAtoms.cpp, the portable branch) as plain functions: the
// float derivation of an atom's parameters, one atom sample, the queue's due test and position advance, and the book player's
// schedule.  No device state: the same text compiles for the host (mxg_atoms_*_host, tests/host_atoms.cpp) and for the kernels of
// atoms.hip (K22).
//
// maxiCollider::createGabor (A = maxiAtoms.cpp; A:27-89), all float but the window:
//     atom[i] = (float)env[i]                          env = the gaussian window of that length (maxiGrains.h:75-123), doubles
//     cycleLen = sampleRate / freq;  maxPhase = length / cycleLen;  inc = 1.0 / length  (a double quotient rounded to float)
//     maxPhase *= TWOPI                                (a double product rounded to float)
//     x = inc * i;  s = sin((x * maxPhase) + startPhase)   -- a float argument: sinf
//     atom[i] *= s;  atom[i] *= amp
// Everything but the sine is the same float operations here (the library is built without contraction).  The sine is atoms_sin on
// the float argument widened to double, rounded once to float: see there.
//
// maxiAccelerator::fillNextBuffer (A:105-126): an entry is due if (int)(startTime + pos) lies in [sampleIdx, sampleIdx + n); a due entry
// adds min(n, size - pos) samples from buffer[0] on and advances pos by as many; an entry whose pos has reached its size is erased,
// due or not.  maxiAtomBookPlayer::play (A:198-219): player_limit / player_offset below.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

#if defined(__HIPCC__) || defined(__clang__)
#define MXG_ATOMS_NO_CONTRACT _Pragma("clang fp contract(off)")
#define MXG_ATOMS_NO_CONTRACT_ATTR
#else  // g++ (tests/host_atoms.cpp): the same, as a function attribute
#define MXG_ATOMS_NO_CONTRACT
#define MXG_ATOMS_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#endif

// include/maxigpu.h, where it is included, comes first and has these
#ifndef MXG_ATOM_KINDS
#define MXG_ATOM_GABOR 0
#define MXG_ATOM_RAW 1
#define MXG_ATOM_KINDS 2
#define MXG_ATOM_ONSET_BLOCK 0
#define MXG_ATOM_ONSET_SAMPLE 1
#define MXG_ATOMS_PIECE 64
#endif

namespace mxg {
namespace {

// ---- the sine -----------------------------------------------------------------------------------------------------------------------
// sin(x) for a double x that holds a FLOAT (24 significant bits), |x| <= 2^19: the arguments of createGabor reach 6.3e4 rad (22 049
// samples at 20 kHz), far beyond sin_small's |x| <= 64 (mxg_sincos.h).  x = fn*pi/2 + (y + t) with pi/2 in the three 33-bit pieces of
// fdlibm's e_rem_pio2.c and their tail: fn has at most 19 bits, so every fn*piece product is exact (33 + 19 <= 53 bits), x - fn*hi is
// exact (Sterbenz), and the two further subtractions are error-free TwoSums -- y + t = x - fn*pi/2 to about 2^-100 absolute, far
// below an ULP of the result even for the floats next to a multiple of pi/2 (a 24-bit argument cannot come very close to one).
// Then fdlibm's minimax kernels for sin and cos on [-pi/4, pi/4] (k_sin.c / k_cos.c: the coefficient sets below), whose documented
// error is below 1 ULP.  Every step is a single IEEE-754 operation (+ - * fma rint) in a fixed order with contraction OFF, the
// Horner chains spelled as fma(): host and device builds give the same bits.  Measured against quad precision by tests/host_atoms.cpp
// on 3.3 M float arguments, the two floats next to every multiple of pi/2 below 2^19 among them: 0.77 ULP at most, and the float it
// rounds to is the nearest float to the true sine on every one of them.
namespace atoms_detail {
constexpr double kInvPio2 = 6.36619772367581382433e-01;
constexpr double kPio2_1 = 1.57079632673412561417e+00, kPio2_2 = 6.07710050630396597660e-11, kPio2_3 = 2.02226624871116645580e-21,
                 kPio2_3t = 8.47842766036889956997e-32;
constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
}  // namespace atoms_detail
constexpr float kAtomsMaxArg = 524288.0f;  // 2^19: the refusal bound on |maxPhase| + |startPhase|

MXG_ATOMS_NO_CONTRACT_ATTR MXG_HD double atoms_sin(double x) {
    MXG_ATOMS_NO_CONTRACT
    using namespace atoms_detail;
    const double fn = rint(x * kInvPio2);
    const double r1 = x - fn * kPio2_1;  // exact
    const double w2 = fn * kPio2_2;      // exact
    const double r2 = r1 - w2, b2 = r1 - r2, e2 = (r1 - (r2 + b2)) + (b2 - w2);
    const double w3 = fn * kPio2_3;      // exact
    const double r3 = r2 - w3, b3 = r2 - r3, e3 = (r2 - (r3 + b3)) + (b3 - w3);
    const double tail = (e2 + e3) - fn * kPio2_3t;
    const double y = r3 + tail;
    const double t = (r3 - y) + tail;
    const int n = (int)fn & 3;
    const double z = y * y;
    double r;
    if (n & 1) {  // cos(y + t)
        const double p = z * fma(z, fma(z, fma(z, fma(z, fma(z, C6, C5), C4), C3), C2), C1);
        const double hz = 0.5 * z, w = 1.0 - hz;
        r = w + (((1.0 - w) - hz) + (z * p - y * t));
    } else {  // sin(y + t)
        const double v = z * y;
        const double p = fma(z, fma(z, fma(z, fma(z, S6, S5), S4), atoms_detail::S3), S2);  // (S3 qualified: mxg_scan.h has a struct of that name)
        r = y - ((z * (0.5 * t - v * p) - t) - v * S1);
    }
    return (n & 2) ? -r : r;
}

// ---- createGabor ----------------------------------------------------------------------------------------------------------------------
struct GaborPar {
    float inc, maxPhase;
};
// A:58-60, :78.  `1.0 / length` and `maxPhase * TWOPI` are double operations rounded to float, the rest float.
MXG_ATOMS_NO_CONTRACT_ATTR MXG_HD GaborPar gabor_params(float freq, float sampleRate, unsigned length) {
    MXG_ATOMS_NO_CONTRACT
    const float cycleLen = sampleRate / freq;
    float maxPhase = length / cycleLen;
    const float inc = (float)(1.0 / length);
    maxPhase = (float)(maxPhase * 6.283185307179586476925286766559);
    return {inc, maxPhase};
}
// What maxiAtomBookPlayer::play hands to createGabor for a book atom (A:211): linlin(frequency, 0, 1, 20, 20000) and amp / 40.0 are
// doubles that the float parameters round; the sample rate is 44100 whatever maxiSettings says.
MXG_ATOMS_NO_CONTRACT_ATTR MXG_HD float book_freq(float frequency) {
    MXG_ATOMS_NO_CONTRACT
    double val = frequency;
    val = val < 1.0 ? val : 1.0;  // max(min(val, inMax), inMin), maximilian.h:803
    val = val < 0.0 ? 0.0 : val;
    return (float)(((val - 0.0) / (1.0 - 0.0) * (20000.0 - 20.0)) + 20.0);
}
MXG_HD float book_amp(float amp) { return (float)(amp / 40.0); }
constexpr float kBookSampleRate = 44100.0f;

// atom[i]: env_f = (float)env[i]
MXG_ATOMS_NO_CONTRACT_ATTR MXG_HD float gabor_sample(float env_f, float inc, float maxPhase, float startPhase, float amp, unsigned i) {
    MXG_ATOMS_NO_CONTRACT
    const float x = inc * i;
    const float arg = (x * maxPhase) + startPhase;
    const float s = (float)atoms_sin((double)arg);
    float a = env_f;
    a *= s;
    a *= amp;
    return a;
}

// the gaussian window (maxiGrains.h:75-92; grains.hip window_value kind 8 is the same expression).  Host only: libm's exp.
inline double gabor_window(unsigned long windowLength, unsigned long windowPos) {
    const double gausDivisor = (-2.0 * 0.3 * 0.3);
    const double phase = ((windowPos / (double)windowLength) - 0.5) * 2.0;
    return exp((phase * phase) / gausDivisor);
}

// ---- the queue ------------------------------------------------------------------------------------------------------------------------
// One queued atom (maxiAccelerator::queuedAtom) with what renders it: GABOR the parameters and the offset of its length's window table,
// RAW the offset of the caller's floats in the raw pool.
struct AtomInst {
    int64_t startTime;
    uint32_t pos, size;
    uint32_t kind, off;
    float inc, maxPhase, startPhase, amp;
};
// One due atom's share of one block: count samples from atom[src_pos] on, added to buffer[dst_off] on.
struct AtomSeg {
    uint32_t kind, off, src_pos, dst_off, count;
    float inc, maxPhase, startPhase, amp;
};
constexpr int kAtomSegWords = sizeof(AtomSeg) / 4;

// A:108-110.  `int atomStart = startTime + pos` narrows to int as x86-64 does; the comparisons are in long.
MXG_HD bool atom_due(int64_t startTime, uint32_t pos, int64_t sampleIdx, uint32_t n, int32_t &atomStart) {
    atomStart = (int32_t)(uint32_t)((uint64_t)startTime + pos);
    return (int64_t)atomStart >= sampleIdx && (int64_t)atomStart < sampleIdx + (int64_t)n;
}
// A:112-116 for a due entry: the samples it adds to this block and where.  BLOCK: from buffer[0] (the reference).  SAMPLE (extension):
// from its own sample, atomStart - sampleIdx, and no further than the block.
MXG_HD uint32_t atom_advance(uint32_t pos, uint32_t size, uint32_t n, int onset, int32_t atomStart, int64_t sampleIdx, uint32_t &dst_off) {
    dst_off = onset == MXG_ATOM_ONSET_SAMPLE ? (uint32_t)((int64_t)atomStart - sampleIdx) : 0u;
    const int room = (int)(n - dst_off), left = (int)(size - pos);
    const int renderLength = room < left ? room : left;
    return renderLength > 0 ? (uint32_t)renderLength : 0u;
}

// ---- the book player ------------------------------------------------------------------------------------------------------------------
// A:200-209: looped = idx % numSamples; atomIdx returns to 0 when looped < bufferSize; atoms are scheduled while
// atom->position < (idx + bufferSize) % numSamples -- a float against a long, compared in float.
MXG_HD int32_t player_looped(int64_t idx, uint32_t numSamples) { return (int32_t)(idx % (int64_t)numSamples); }
MXG_HD float player_limit(int64_t idx, uint32_t n, uint32_t numSamples) { return (float)((idx + (int64_t)n) % (int64_t)numSamples); }
// A:212 `addAtom(atomData, loopedSamplePos - atom->position)`: a float converted to unsigned.  Where that float is non-negative this is
// the reference's value.  Where it is negative the reference's conversion is undefined (on x86-64 the atom lands 2^32 samples ahead
// and never sounds); the evident intent is position - looped, the atom's distance into this block, and that is what this returns:
// |looped - position|.
MXG_HD uint32_t player_offset(int32_t looped, float position) {
    float d = looped - position;
    if (d < 0.0f) d = -d;
    return (uint32_t)d;
}

// The host form of one stream's step (mxg_atoms_*_host): optionally the player's step, then the walk over the live list in queue order.
// Returns the number of segments written to seg[] (at most Q), or -1 on overflow of the live list (nothing is changed then).
struct AtomBookView {
    const float *position;  // [n]
    const AtomInst *inst;   // [n]: startTime and pos unset
    uint32_t n, numSamples;
};
inline int atoms_stream_step(bool player, const AtomBookView &book, int onset, uint32_t N, size_t Q, int64_t &sampleIdx, uint32_t &atomIdx,
                             int32_t &nlive, AtomInst *live, AtomSeg *seg) {
    const int64_t idx = sampleIdx;
    uint32_t ai = atomIdx, end = atomIdx;
    if (player) {
        const int32_t looped = player_looped(idx, book.numSamples);
        if ((int64_t)looped < (int64_t)N) ai = 0;
        const float limit = player_limit(idx, N, book.numSamples);
        end = ai;
        while (end < book.n && book.position[end] < limit) end++;
        if ((size_t)nlive + (end - ai) > Q) return -1;
        for (uint32_t k = ai; k < end; k++) {
            AtomInst a = book.inst[k];
            a.startTime = idx + (int64_t)player_offset(looped, book.position[k]);
            a.pos = 0;
            live[nlive++] = a;
        }
    }
    int nseg = 0, keep = 0;
    for (int k = 0; k < nlive; k++) {
        AtomInst a = live[k];
        int32_t atomStart;
        if (atom_due(a.startTime, a.pos, idx, N, atomStart)) {
            uint32_t dst;
            const uint32_t cnt = atom_advance(a.pos, a.size, N, onset, atomStart, idx, dst);
            if (cnt) seg[nseg++] = {a.kind, a.off, a.pos, dst, cnt, a.inc, a.maxPhase, a.startPhase, a.amp};
            a.pos += cnt;
        }
        if (a.pos != a.size) live[keep++] = a;
    }
    nlive = keep;
    atomIdx = end;
    sampleIdx = idx + (int64_t)N;
    return nseg;
}

// one segment into a stream's block, sample after sample (the host form of the render)
inline void atoms_seg_render(const AtomSeg &g, const float *win, const float *raw, float *buf) {
    for (uint32_t d = 0; d < g.count; d++) {
        const uint32_t i = g.src_pos + d;
        const float v = g.kind == MXG_ATOM_RAW ? raw[(size_t)g.off + i] : gabor_sample(win[(size_t)g.off + i], g.inc, g.maxPhase, g.startPhase, g.amp, i);
        buf[g.dst_off + d] = buf[g.dst_off + d] + v;
    }
}

}  // namespace
}  // namespace mxg
