// mxg_analysis.h -- the reference's time-domain analysis classes as plain per-sample arithmetic over small state structs:
// maxiZeroCrossingDetector::zx (H:1002-1011), maxiZeroCrossingRate::play (H:1025-1034) over maxiRingBuf (H:424-494),
// maxiEnvelopeFollowerType<T>::play (H:1232-1240) and maxiSampleAndHold::sah (H:973-985).  H = src/maximilian.h.  No device
// state: the same text compiles for the host (tests/host_analysis.cpp, the drop-in classes of include/maximilian.h).
// Everything is compares, + - *, integer counts and indexing: bit-exact, no tolerance anywhere.
//
// What is reproduced is what the reference computes:
//   * zx: res = (prev <= 0 && x > 0); prev = x.  NaN and -0.0 follow from the two compares (a NaN never crosses and, as prev,
//     never lets the next sample cross; -0.0 <= 0 holds);
//   * the rate: push the crossing at idx, idx++ wrapping at the ring's size, count += bit, count -= tail(W) with tail() looked
//     up AFTER the push (W == size: the slot the next push overwrites; W == 1: the bit just pushed, the count stays 0);
//   * the follower: a = fabs(x); env = (a > env ? attack : release) * (env - a) + a, never contracted into an FMA;
//   * sample and hold: hold = (double)(size_t)(ms / 1000.0 * sampleRate) at every sample; phase >= hold subtracts hold ONCE;
//     phase < 1 samples; hold == 0 therefore samples only on the object's very first call.
// The ring of crossings holds one BIT per slot: slot s is bit s & 63 of word s >> 6, words word-major (ring[word * stride]).
// The head word (the slot the next push writes) and the tail word are cached; a word goes to memory when the head leaves it.
// Two defined departures: a window above the ring's size is held at the size (the caller counts it), where the reference
// indexes out of bounds; the count is a signed 64-bit integer, where the reference's size_t would pass through a negative
// double when the window changes over a filled ring.  A negative or NaN hold time is 0 samples (undefined in the reference).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mxg_hd.h"

#define MXG_ANA_WANT_ZX 1
#define MXG_ANA_WANT_ZCR 2
#define MXG_ANA_WANT_ENV 4
#define MXG_ANA_WANT_SAH 8
#define MXG_ANA_WANT_ALL 15

namespace mxg {
namespace {

// ---- maxiZeroCrossingDetector::zx ------------------------------------------------------------------------------------
MXG_HD bool ana_zx(double &prev, double x) {
    const bool res = prev <= 0 && x > 0;
    prev = x;
    return res;
}

// ---- maxiZeroCrossingRate::play over a ring of bits ------------------------------------------------------------------
struct AnaZcr {
    uint64_t *ring;   // this voice's column: word w at ring[w * stride]
    size_t stride;
    int cap, window;  // slots; 1 <= window <= cap
    int idx;          // maxiRingBuf::idx, the slot the next push writes
    long long count;  // runningCount
    uint64_t head, tail;  // cached words
    int hw, tw;           // their word indices; tw < 0: nothing cached
    bool live;            // false: a shadow lane, computes and stores nothing
};

MXG_HD size_t ana_ring_words(size_t cap) { return (cap + 63) >> 6; }

MXG_HD void ana_zcr_open(AnaZcr &z) {
    z.hw = z.idx >> 6;
    z.head = z.ring[(size_t)z.hw * z.stride];
    z.tw = -1;
    z.tail = 0;
}

MXG_HD double ana_zcr_step(AnaZcr &z, bool bit) {
    const uint64_t m = (uint64_t)1 << (z.idx & 63);
    z.head = bit ? (z.head | m) : (z.head & ~m);
    int idx = z.idx + 1;
    if (idx == z.cap) idx = 0;
    z.idx = idx;
    const int nhw = idx >> 6;
    if (nhw != z.hw) {  // the head leaves its word: the word goes to memory, and replaces a cached tail copy of the same word
        if (z.live) z.ring[(size_t)z.hw * z.stride] = z.head;
        if (z.tw == z.hw) z.tail = z.head;
        z.hw = nhw;
        z.head = z.ring[(size_t)nhw * z.stride];
    }
    const int t = idx >= z.window ? idx - z.window : z.cap - (z.window - idx);  // maxiRingBuf::tail, after the push
    const int tw = t >> 6;
    uint64_t w;
    if (tw == z.hw) {
        w = z.head;  // one copy where head and tail share a word
    } else {
        if (tw != z.tw) {
            z.tail = z.ring[(size_t)tw * z.stride];
            z.tw = tw;
        }
        w = z.tail;
    }
    z.count += bit ? 1 : 0;
    z.count -= (long long)((w >> (t & 63)) & 1);
    return (double)z.count;
}

MXG_HD void ana_zcr_close(AnaZcr &z) {
    if (z.live) z.ring[(size_t)z.hw * z.stride] = z.head;
}

// ---- maxiEnvelopeFollowerType<T>::play -------------------------------------------------------------------------------
template <typename T>
MXG_HD T ana_follow(T &env, T attack, T release, T x) {
    const T a = (T)fabs(x);  // (the reference's fabs is the double one for both instantiations; |x| is exact either way)
    if (a > env) env = attack * (env - a) + a;
    else env = release * (env - a) + a;
    return env;
}

// ---- maxiSampleAndHold::sah ------------------------------------------------------------------------------------------
// (double)(size_t)t for t in [0, 2^64): trunc(t) is that value exactly; a negative or NaN time is 0 samples
MXG_HD double ana_hold_samples(double ms, double sr) {
    const double t = ms / 1000.0 * sr;
    return t >= 1.0 ? trunc(t) : 0.0;
}
MXG_HD double ana_sah(double &phase, double &value, double x, double hold) {
    if (phase >= hold) phase -= hold;
    if (phase < 1.0) value = x;
    phase++;
    return value;
}

}  // namespace
}  // namespace mxg
