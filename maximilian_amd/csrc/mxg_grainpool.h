// mxg_grainpool.h -- K27's arithmetic: granular streams that each read their OWN slot of a sample pool (maxiTimeStretch /
// maxiPitchShift / maxiStretch with setSample, L/maxiGrains.h), maxiStretch's loop points (:445, :493-509, :514-517) and
// maxiStretch::playAtPosition (:531-539), with speed, rate, position and posMod readable at every sample.  Plain arithmetic on
// doubles and integers, host + device: grainpool.hip's kernel runs gp_walk_stream one lane per stream, the library's
// mxg_granular_pool_host and tests/host_grainpool.cpp run the same text on the host.  The scheduler state, the birth of a grain and
// the rand() draws are mxg_sched.h's (SchedState, grain_birth, sched_draw, sched_step), included and left as they are.
//
// Modes: 0 maxiTimeStretch::play, 1 maxiStretch::play (with loop points), 2 maxiTimeStretch::playAtPosition,
// 3 maxiPitchShift::play, 4 maxiStretch::playAtPosition.
//   a: modes 0/3 speed, 1/4 pitchstretch: [S], or [T][S] under MXG_GPOOL_PS_A; mode 2: the position signal, always [T][S]
//   b: mode 1 timestretch, mode 4 the position: [S], or [T][S] under MXG_GPOOL_PS_B
//   posMod (modes 0/1/3): null, [S], or [T][S] under MXG_GPOOL_PS_POSMOD
// A per-sample value is what a patch passes to play() in that sample: speed / rate move `position` at every sample, a grain takes
// the values of the sample it is born in.
#pragma once
#include "mxg_hd.h"
#include "mxg_sched.h"

#ifndef MXG_GPOOL_PS_A
#define MXG_GPOOL_PS_A 1
#define MXG_GPOOL_PS_B 2
#define MXG_GPOOL_PS_POSMOD 4
#endif

namespace mxg {

// one call (the pointers are host or device arrays alike)
struct GpArgs {
    size_t S, T, R, stride, cap, Rn;
    const double *pool;      // element 0 of slot 0
    const uint64_t *len;     // [R]
    const uint32_t *slot;    // [S] or null (stream s reads slot s)
    const uint64_t *loop;    // [2][S] loopStart | loopEnd, or null (0, len)
    const double *window;    // [sampleDur]
    const double *a, *b, *posMod;
    int ps;
    const int32_t *rnd;      // [S][Rn] or null
    double *st, *gst, *out;  // [4][S], [4][8][S], [T][S]
    double sr, cycleLength, grainLength;
    int sampleDur;
};

namespace {

constexpr int kGpSlots = 8;  // live grains per stream (the ceiling of mxg_granular_render)
// the codes of a stream's failure (the async error word adds ASYNC_GRAIN_BASE): as in grains.hip
constexpr int kGpTooMany = 1, kGpRndExhausted = 2, kGpForeign = 4, kGpStep = 5;

// maxiStretch's members loopStart / loopEnd / loopLength are unsigned long; play() compares and adds them to the double
// `position` (:516-517), i.e. converted to double.  loopLength = loopEnd - loopStart in unsigned arithmetic (:495, :500).
struct GpLoop {
    double loopStart, loopEnd, loopLength;
};
MXG_DEV GpLoop gp_loop(uint64_t loopStart, uint64_t loopEnd) {
    GpLoop l;
    l.loopStart = (double)loopStart;
    l.loopEnd = (double)loopEnd;
    l.loopLength = (double)(uint64_t)(loopEnd - loopStart);
    return l;
}

// One sample of the scheduler.  c holds this sample's speed / rate / pm; bpos is mode 4's position argument.
// Modes 0, 2 and 3 are sched_step itself.
template <int MODE>
MXG_DEV bool gp_sched_step(SchedState &q, const SchedConst &c, const GpLoop &lp, const double bpos, size_t n,
                           double &pos0, double &inc, int &failed) {
    if constexpr (MODE == 1) {  // maxiStretch::play :514-526
        q.position = q.position + c.rate;
        q.looper += 1.0;
        if (q.position >= lp.loopEnd) q.position -= lp.loopLength;
        if (q.position < lp.loopStart) q.position += lp.loopLength;
        if (q.looper > q.thr) {
            sched_spawn01<1>(q, c, pos0, inc, failed);
            return true;
        }
        return false;
    } else if constexpr (MODE == 4) {  // maxiStretch::playAtPosition :531-539
        q.looper += 1.0;
        double pos = bpos;
        pos *= c.dlen;
        if (0 == floor(fmod(q.looper, c.cycleLength))) {
            grain_birth(c, (pos / c.dlen), c.speed, pos0, inc, failed);
            return true;
        }
        return false;
    } else {
        return sched_step<MODE>(q, c, n, pos0, inc, failed);
    }
}

// a live grain handed in through gst must be one this plan could have made in THIS stream's slot (grains.hip carried_grain_ok)
MXG_DEV bool gp_carried_ok(double pos, double inc, double idx, double dur, double dlen, int sampleDur) {
    return dur == (double)sampleDur && idx >= 0.0 && idx < dur && pos >= 0.0 && pos <= dlen && fabs(inc) <= dlen;
}

// maxiGrain::play :216-245 without the window: moves pos, returns the interpolated sample.  pos stays inside [0, len]; the one
// value outside [0, len) -- pos + len rounding up to len exactly after a wrap from below zero -- reads the zero an uploaded
// sample and a pool slot keep behind their last element (the oracle's guard element), without touching memory.
MXG_DEV double gp_grain_read(double &gpos, const double ginc, const double dlen, const size_t len,
                             const double *buf) {
    double pos = gpos + ginc;
    if (pos >= dlen)
        pos -= dlen;
    else if (pos < 0)
        pos += dlen;
    gpos = pos;
    const double fl = floor(pos);
    const double remainder = pos - fl;
    const size_t ia = (size_t)(long long)fl;
    size_t ib = ia + 1;
    if (ib >= len) ib = 0;
    const double va = ia < len ? buf[ia] : 0.0;
    return ((1 - remainder) * va + remainder * buf[ib]);
}

// What a stream's scheduler needs for a call: its slot, loop and the parameters a sample reads.
template <int MODE>
struct GpStream {
    size_t len;
    const double *buf;
    double dlen, av, bv;
    GpLoop lp;
    SchedConst sc;
    bool psA, psB, psP;
    // false: a slot index outside the pool or an empty slot
    MXG_DEV bool setup(const GpArgs &A, const size_t s) {
        const size_t S = A.S;
        const size_t r = A.slot ? (size_t)A.slot[s] : s;
        uint64_t l64 = r < A.R ? A.len[r] : 0;
        if (l64 > A.cap) l64 = A.cap;
        len = (size_t)l64;
        if (len == 0) return false;
        buf = A.pool + r * A.stride;
        dlen = (double)len;
        uint64_t ls = 0, le = l64;
        if (MODE == 1 && A.loop) {
            ls = A.loop[s];
            le = A.loop[S + s];
        }
        lp = gp_loop(ls, le);
        sc.dlen = dlen;
        sc.cycleLength = A.cycleLength;
        sc.grainLength = A.grainLength;
        sc.sr = A.sr;
        sc.sampleDur = A.sampleDur;
        sc.a_ps = A.a + s;
        sc.S = S;
        sc.rnd = A.rnd ? A.rnd + s * A.Rn : nullptr;
        sc.R = A.Rn;
        psA = MODE != 2 && (A.ps & MXG_GPOOL_PS_A);
        psB = (MODE == 1 || MODE == 4) && (A.ps & MXG_GPOOL_PS_B);
        psP = (MODE == 0 || MODE == 1 || MODE == 3) && A.posMod && (A.ps & MXG_GPOOL_PS_POSMOD);
        av = (MODE == 2 || psA) ? 1.0 : A.a[s];
        bv = ((MODE == 1 || MODE == 4) && !psB) ? A.b[s] : 0.0;
        sc.pm = ((MODE == 0 || MODE == 1 || MODE == 3) && A.posMod && !psP) ? A.posMod[s] : 0.0;
        sc.speed = av;
        sc.rate = MODE == 1 ? bv : av;
        return true;
    }
    // the arguments play() is handed in sample n
    MXG_DEV void sample(const GpArgs &A, const size_t s, const size_t n) {
        if (psA) {
            av = A.a[n * A.S + s];
            sc.speed = av;
            if (MODE != 1) sc.rate = av;
        }
        if (psB) {
            bv = A.b[n * A.S + s];
            if (MODE == 1) sc.rate = bv;
        }
        if (psP) sc.pm = A.posMod[n * A.S + s];
    }
};

// The whole of stream s for A.T samples: K27's walk.  win = the window table (the kernel stages it in LDS).  Returns the
// stream's failure code (0 = none).
template <int MODE>
MXG_DEV int gp_walk_stream(const GpArgs &A, const size_t s, const double *win) {
    const size_t S = A.S;
    int failed = 0;
    double *op = A.out + s;
    GpStream<MODE> g;
    if (!g.setup(A, s)) {  // nothing is read, the state stays, the output is silence
        for (size_t n = 0; n < A.T; n++) op[n * S] = 0.0;
        return kGpStep;
    }
    const size_t len = g.len;
    const double *buf = g.buf;
    const double dlen = g.dlen;
    SchedState q = {A.st[s], A.st[S + s], A.st[2 * S + s], 0.0, (size_t)A.st[3 * S + s]};
    q.thr = A.cycleLength + q.randomOffset;

    double gpos[kGpSlots], ginc[kGpSlots];
    int gidx[kGpSlots], gdur[kGpSlots];
    int tail = 0;
#pragma unroll
    for (int k = 0; k < kGpSlots; k++) {
        gpos[k] = A.gst[(0 * kGpSlots + k) * S + s];
        ginc[k] = A.gst[(1 * kGpSlots + k) * S + s];
        const double idx = A.gst[(2 * kGpSlots + k) * S + s], dur = A.gst[(3 * kGpSlots + k) * S + s];
        if (dur != 0.0 && !gp_carried_ok(gpos[k], ginc[k], idx, dur, dlen, A.sampleDur)) {
            failed = kGpForeign;
            gidx[k] = 0;
            gdur[k] = 0;
        } else {
            gidx[k] = (int)idx;
            gdur[k] = (int)dur;
        }
        if (gdur[k]) tail = k + 1;
    }
    for (size_t n = 0; n < A.T; n++) {
        g.sample(A, s, n);
        double bornPos, bornInc;
        if (gp_sched_step<MODE>(q, g.sc, g.lp, g.bv, n, bornPos, bornInc, failed)) {
            if (tail == kGpSlots) {  // compact the holes
#pragma unroll
                for (int pass = 0; pass < kGpSlots - 1; pass++)
#pragma unroll
                    for (int k = 0; k < kGpSlots - 1; k++)
                        if (gdur[k] == 0) {
                            gpos[k] = gpos[k + 1]; ginc[k] = ginc[k + 1]; gidx[k] = gidx[k + 1];
                            gdur[k] = gdur[k + 1]; gdur[k + 1] = 0;
                        }
                tail = 0;
#pragma unroll
                for (int k = 0; k < kGpSlots; k++)
                    if (gdur[k]) tail = k + 1;
            }
            if (tail == kGpSlots) {
                failed = kGpTooMany;  // more than 8 grains alive: the grain is dropped, the stream keeps running
            } else {
#pragma unroll
                for (int k = 0; k < kGpSlots; k++)
                    if (k == tail) {
                        gpos[k] = bornPos; ginc[k] = bornInc; gidx[k] = 0; gdur[k] = A.sampleDur;
                    }
                tail++;
            }
        }
        // maxiGrainPlayer::play :270-283: the live grains in creation order
        double total = 0.0;
#pragma unroll
        for (int k = 0; k < kGpSlots; k++) {
            if (gdur[k] > 0) {
                const double envValue = win[gidx[k]];
                double o = gp_grain_read(gpos[k], ginc[k], dlen, len, buf);
                o *= envValue;
                total += o;
                gidx[k]++;
                if (gidx[k] == gdur[k]) gdur[k] = 0;
            }
        }
        if (tail > 0 && gdur[0] == 0) {  // the oldest grain is gone: close ranks
#pragma unroll
            for (int k = 0; k < kGpSlots - 1; k++) {
                gpos[k] = gpos[k + 1]; ginc[k] = ginc[k + 1]; gidx[k] = gidx[k + 1]; gdur[k] = gdur[k + 1];
            }
            gdur[kGpSlots - 1] = 0;
            tail--;
        }
        op[n * S] = total;
    }
    A.st[s] = q.position;
    A.st[S + s] = q.looper;
    A.st[2 * S + s] = q.randomOffset;
    A.st[3 * S + s] = (double)q.cursor;
#pragma unroll
    for (int pass = 0; pass < kGpSlots - 1; pass++)
#pragma unroll
        for (int k = 0; k < kGpSlots - 1; k++)
            if (gdur[k] == 0) {
                gpos[k] = gpos[k + 1]; ginc[k] = ginc[k + 1]; gidx[k] = gidx[k + 1];
                gdur[k] = gdur[k + 1]; gdur[k + 1] = 0;
            }
#pragma unroll
    for (int k = 0; k < kGpSlots; k++) {
        const bool live = gdur[k] > 0;
        A.gst[(0 * kGpSlots + k) * S + s] = live ? gpos[k] : 0.0;
        A.gst[(1 * kGpSlots + k) * S + s] = live ? ginc[k] : 0.0;
        A.gst[(2 * kGpSlots + k) * S + s] = live ? (double)gidx[k] : 0.0;
        A.gst[(3 * kGpSlots + k) * S + s] = live ? (double)gdur[k] : 0.0;
    }
    return failed;
}

// ---- the tile form: a scheduler pass and a render pass ---------------------------------------------------------------------------
// The only serial part of a stream is its scheduler.  gp_tile_sched runs it (one lane per stream, the one-sample step -- which is
// what lets every parameter change at every sample), records every grain born (sample, start position, step), how many births
// precede every tile of 64 samples, a copy of the grains carried in, and leaves the state of the call's END: the scheduler's, and
// the grains alive then, advanced from their birth with the exact multi-step forms of mxg_advance.h.  gp_tile_sample then gives
// sample n of stream s on its own: a grain's recurrence restarts at its birth, so its position at the tile's start is an anchor
// (gp_advance: advance_until between wraps) and the 64 steps inside the tile are a line on the mantissa grid (add_line), which a
// lane evaluates for its own sample.  Wherever the line form does not hold -- a wrap or a binade crossing inside the tile, a
// step <= 0, a tie -- the lane walks its steps from the anchor one by one: the same additions in the same order either way.
// births a stream can record in T samples: one per cycle at most (randomOffset only lengthens a cycle; a cycle under one sample
// is a birth per sample)
static inline size_t gp_lists_births(size_t T, double cycleLength) {
    const double c = cycleLength > 1.0 ? floor(cycleLength) : 1.0;
    return (size_t)((double)T / c) + 2;
}
struct GpLists {
    size_t G, C;          // births a stream can record; tiles of 64 samples
    int32_t *birth_n;     // [G][S]
    double *birth_pos;    // [G][S]
    double *birth_inc;    // [G][S]
    int32_t *first;       // [C + 1][S]: births before sample 64 c
    double *gst_in;       // [4][8][S]: the grains carried in (gst itself receives the grains carried out)
};
constexpr int kGpTile = 64;
constexpr int kGpListOverflow = 3;

// The mirror of advance_until's binade case for a NEGATIVE step: x <- fl(x - r), x >= 0, r > 0, at most kmax steps, stopping right
// after the first step that leaves x < 0.  Inside x's binade [2^e, 2^(e+1)) every partial difference that stays ABOVE 2^e is a
// multiple of u = 2^(e-52); r = (R + f) u, and round-to-nearest (symmetric in sign) takes off R ulps (f < 1/2) or R + 1 (f > 1/2)
// on every step: X_k = X - k c.  The jump stops one ulp short of 2^e -- at 2^e itself the exact difference lies on the finer grid
// below -- and the tie f == 1/2, the step across the binade's lower edge, zero, subnormals and the crossing step are plain steps.
MXG_DEV int gp_retreat_until(double &x, const double r, const int kmax, bool &crossed) {
    crossed = false;
    int done = 0;
    while (done < kmax) {
        bool jumped = false;
        const long long xb = __double_as_longlong(x);
        const int e = (int)((xb >> 52) & 0x7ff), er = (int)((__double_as_longlong(r) >> 52) & 0x7ff);
        if (xb > 0 && e > 0 && e < 0x7ff && er > 0 && er < 0x7ff) {
            const double ru = ldexp(r, 1075 - e);  // r in ulps of x (exact scaling; may underflow to 0: f then < 1/2)
            if (ru < 4503599627370496.0) {
                const double Rf = floor(ru), fr = ru - Rf;
                if (fr != 0.5) {
                    const long long c = (long long)Rf + (fr > 0.5 ? 1 : 0);
                    const long long X = (xb & 0xFFFFFFFFFFFFFLL) | (1LL << 52);
                    long long j = (long long)(kmax - done);
                    const long long room = X - ((1LL << 52) + 1);
                    if (room < 0) {
                        j = 0;  // x = 2^e itself: the grid below it is finer, a plain step
                    } else if (c > 0) {
                        const long long jb = floor_div53(room, c);
                        j = jb < j ? jb : j;
                    }  // (c == 0 above the edge: r is under half an ulp, x does not move for any number of steps)
                    if (j >= 1) {
                        const long long Xn = X - j * c;
                        x = __longlong_as_double(((long long)e << 52) | (Xn & 0xFFFFFFFFFFFFFLL));
                        done += (int)j;
                        jumped = true;
                    }
                }
            }
        }
        if (!jumped) {
            x = x - r;
            done++;
            if (x < 0) {
                crossed = true;
                return done;
            }
        }
    }
    return done;
}

// pos after `steps` calls of maxiGrain::play's `pos += inc` with its wrap (:224-228), from a pos inside [0, dlen]: between two wraps
// the exact multi-step forms (advance_until upwards, gp_retreat_until downwards), the wrap itself and whatever they exclude as the
// plain step.  The same additions in the same order as the walk's, whatever the sign of the step.
MXG_DEV double gp_advance(double pos, const double inc, const double dlen, int steps) {
    if (inc > 0.0 && pos >= 0.0) {
        while (steps > 0) {
            bool wrapped;
            steps -= advance_until(pos, inc, dlen, true, steps, wrapped);
            if (wrapped) pos -= dlen;
        }
        return pos;
    }
    if (inc < 0.0 && pos >= 0.0) {
        const double r = -inc;
        while (steps > 0) {
            if (pos >= dlen) {  // (pos == dlen: a grain born at the slot's end, or a wrap from below that rounded up to it)
                pos = pos + inc;
                if (pos >= dlen)
                    pos -= dlen;
                else if (pos < 0)
                    pos += dlen;
                steps--;
                continue;
            }
            bool wrapped;
            steps -= gp_retreat_until(pos, r, steps, wrapped);
            if (wrapped) pos += dlen;
        }
        return pos;
    }
    for (int i = 0; i < steps; i++) {
        pos = pos + inc;
        if (pos >= dlen)
            pos -= dlen;
        else if (pos < 0)
            pos += dlen;
        if (inc == 0.0) break;  // (a step of zero: after the first call's wrap check nothing moves)
    }
    return pos;
}

template <int MODE>
MXG_DEV int gp_tile_sched(const GpArgs &A, const GpLists &L, const size_t s) {
    const size_t S = A.S;
    const int T = (int)A.T, dur = A.sampleDur;
    int failed = 0;
    GpStream<MODE> g;
    if (!g.setup(A, s)) {  // no births, no grains: the render pass writes silence; st and gst stay
        for (size_t c = 0; c <= L.C; c++) L.first[c * S + s] = 0;
        for (int i = 0; i < 4 * kGpSlots; i++) L.gst_in[(size_t)i * S + s] = 0.0;
        return kGpStep;
    }
    SchedState q = {A.st[s], A.st[S + s], A.st[2 * S + s], 0.0, (size_t)A.st[3 * S + s]};
    q.thr = A.cycleLength + q.randomOffset;
    // the live grains: where each was born (carried in: k - 8, which keeps their order in front of every birth), the last sample
    // it plays in, what it started from and how many steps it had taken then
    int born[kGpSlots], last[kGpSlots], age0[kGpSlots];
    double gpos[kGpSlots], ginc[kGpSlots];
#pragma unroll
    for (int k = 0; k < kGpSlots; k++) {
        double pos = A.gst[(0 * kGpSlots + k) * S + s], inc = A.gst[(1 * kGpSlots + k) * S + s];
        double idx = A.gst[(2 * kGpSlots + k) * S + s], d = A.gst[(3 * kGpSlots + k) * S + s];
        if (d != 0.0 && !gp_carried_ok(pos, inc, idx, d, g.dlen, dur)) {
            failed = kGpForeign;
            d = 0.0;
        }
        if (d == 0.0) pos = inc = idx = 0.0;
        L.gst_in[(0 * kGpSlots + k) * S + s] = pos;
        L.gst_in[(1 * kGpSlots + k) * S + s] = inc;
        L.gst_in[(2 * kGpSlots + k) * S + s] = idx;
        L.gst_in[(3 * kGpSlots + k) * S + s] = d;
        born[k] = k - kGpSlots;
        age0[k] = (int)idx;
        last[k] = d != 0.0 ? dur - (int)idx - 1 : -1;
        gpos[k] = pos;
        ginc[k] = inc;
    }
    int count = 0;
    for (int n = 0; n < T; n++) {
        if ((n & (kGpTile - 1)) == 0) L.first[(size_t)(n / kGpTile) * S + s] = count;
        g.sample(A, s, (size_t)n);
        double bornPos, bornInc;
        if (gp_sched_step<MODE>(q, g.sc, g.lp, g.bv, (size_t)n, bornPos, bornInc, failed)) {
            int free_k = -1;
#pragma unroll
            for (int k = 0; k < kGpSlots; k++)
                if (last[k] < n && free_k < 0) free_k = k;
            if (free_k < 0) {
                failed = kGpTooMany;  // eight grains alive: this one is dropped, as the walk drops it
            } else if ((size_t)count >= L.G) {
                failed = kGpListOverflow;
            } else {
                L.birth_n[(size_t)count * S + s] = n;
                L.birth_pos[(size_t)count * S + s] = bornPos;
                L.birth_inc[(size_t)count * S + s] = bornInc;
                count++;
#pragma unroll
                for (int k = 0; k < kGpSlots; k++)
                    if (k == free_k) {
                        born[k] = n; last[k] = n + dur - 1; age0[k] = 0; gpos[k] = bornPos; ginc[k] = bornInc;
                    }
            }
        }
    }
    for (size_t c = (size_t)(T + kGpTile - 1) / kGpTile; c <= L.C; c++) L.first[c * S + s] = count;
    A.st[s] = q.position;
    A.st[S + s] = q.looper;
    A.st[2 * S + s] = q.randomOffset;
    A.st[3 * S + s] = (double)q.cursor;
    // the grains alive after the call, in creation order
    int prev = -2 * kGpSlots, o = 0;
    for (int pass = 0; pass < kGpSlots; pass++) {
        int pick = -1, key = 0x7fffffff;
        for (int k = 0; k < kGpSlots; k++)
            if (last[k] >= T && born[k] > prev && born[k] < key) {
                key = born[k];
                pick = k;
            }
        if (pick < 0) break;
        prev = key;
        const int steps = key < 0 ? T : T - key;
        A.gst[(0 * kGpSlots + o) * S + s] = gp_advance(gpos[pick], ginc[pick], g.dlen, steps);
        A.gst[(1 * kGpSlots + o) * S + s] = ginc[pick];
        A.gst[(2 * kGpSlots + o) * S + s] = (double)(age0[pick] + steps);
        A.gst[(3 * kGpSlots + o) * S + s] = (double)dur;
        o++;
    }
    for (; o < kGpSlots; o++)
        for (int f = 0; f < 4; f++) A.gst[((size_t)f * kGpSlots + o) * S + s] = 0.0;
    return failed;
}

// one grain's share of sample n0 + j: the grain has taken k0 steps from x when the tile starts (its first step inside the tile is
// lane j0's, at age m0).  Everything but j is the same for the 64 lanes of a tile.
MXG_DEV void gp_tile_grain(double &total, double x, const double inc, const int k0, const int j0, const int m0, const int j,
                           const int dur, const double dlen, const size_t len, const double *buf, const double *win) {
    const double x0 = gp_advance(x, inc, dlen, k0);
    const AddLine line = add_line(x0, inc, dlen, kGpTile);
    const int m = m0 + (j - j0);
    if (j < j0 || m >= dur) return;
    const int t = j - j0 + 1;
    double pos;
    if (line.ok) {
        pos = add_line_at(line, t - 1);  // the anchor for gp_grain_read's own step, the t-th
    } else {
        pos = x0;
        for (int i = 1; i < t; i++) {
            pos = pos + inc;
            if (pos >= dlen)
                pos -= dlen;
            else if (pos < 0)
                pos += dlen;
        }
    }
    double o = gp_grain_read(pos, inc, dlen, len, buf);
    o *= win[m];
    total += o;
}

// out[n0 + j][s], n0 a multiple of 64
MXG_DEV double gp_tile_sample(const GpArgs &A, const GpLists &L, const size_t s, const int n0, const int j,
                              const double *win) {
    const size_t S = A.S;
    const int dur = A.sampleDur;
    const size_t r = A.slot ? (size_t)A.slot[s] : s;
    uint64_t l64 = r < A.R ? A.len[r] : 0;
    if (l64 > A.cap) l64 = A.cap;
    const size_t len = (size_t)l64;
    if (len == 0) return 0.0;
    const double *buf = A.pool + r * A.stride;
    const double dlen = (double)len;
    double total = 0.0;
    for (int k = 0; k < kGpSlots; k++) {  // the grains carried in: they play in samples 0 ... dur - idx - 1
        const double d = L.gst_in[(3 * kGpSlots + k) * S + s];
        if (d == 0.0) continue;
        const int idx = (int)L.gst_in[(2 * kGpSlots + k) * S + s];
        if (idx + n0 >= dur) continue;
        gp_tile_grain(total, L.gst_in[(0 * kGpSlots + k) * S + s], L.gst_in[(1 * kGpSlots + k) * S + s], n0, 0, idx + n0, j, dur, dlen, len, buf, win);
    }
    const int lo = n0 - dur + 1 > 0 ? n0 - dur + 1 : 0;  // a grain born before `lo` is over
    const int i0 = L.first[(size_t)(lo / kGpTile) * S + s], i1 = L.first[(size_t)(n0 / kGpTile + 1) * S + s];
    for (int i = i0; i < i1; i++) {
        const int nb = L.birth_n[(size_t)i * S + s];
        if (nb + dur - 1 < n0) continue;
        const int k0 = nb < n0 ? n0 - nb : 0, j0 = nb > n0 ? nb - n0 : 0;
        gp_tile_grain(total, L.birth_pos[(size_t)i * S + s], L.birth_inc[(size_t)i * S + s], k0, j0, k0, j, dur, dlen, len, buf, win);
    }
    return total;
}

MXG_DEV int gp_walk_stream_mode(int mode, const GpArgs &A, const size_t s, const double *win) {
    switch (mode) {
        case 0: return gp_walk_stream<0>(A, s, win);
        case 1: return gp_walk_stream<1>(A, s, win);
        case 2: return gp_walk_stream<2>(A, s, win);
        case 3: return gp_walk_stream<3>(A, s, win);
        default: return gp_walk_stream<4>(A, s, win);
    }
}

#if !defined(__HIPCC__)  // (a HIP translation unit keeps these functions device-only: grainpool_host.cpp is the host build)
// setLoopStart / setLoopEnd (:493-501): (unsigned long)(val * len).  Returns null, or what is wrong.  The reference's unsigned
// loopLength wraps when loopStart >= loopEnd; that loop is refused here (the one departure).
static inline const char *gp_stretch_loop(uint64_t len, double start01, double end01, uint64_t *loopStart, uint64_t *loopEnd) {
    if (start01 != start01 || end01 != end01) return "a loop point is NaN";
    if (start01 < 0.0 || end01 < 0.0) return "a loop point is negative";
    const double a = start01 * (double)len, b = end01 * (double)len;
    if (!(a < 18446744073709551616.0) || !(b < 18446744073709551616.0)) return "loopEnd is larger than len";
    const uint64_t ls = (uint64_t)a, le = (uint64_t)b;
    if (le > len) return "loopEnd is larger than len";
    if (ls >= le) return "loopStart >= loopEnd";
    *loopStart = ls;
    *loopEnd = le;
    return nullptr;
}

// the call on host arrays in the tile form (scratch lists on the heap of the caller: L sized by gp_lists_*)
static inline int gp_host_render_tiles(int mode, const GpArgs &A, const GpLists &L) {
    int failed = 0;
    for (size_t s = 0; s < A.S; s++) {
        int f;
        switch (mode) {
            case 0: f = gp_tile_sched<0>(A, L, s); break;
            case 1: f = gp_tile_sched<1>(A, L, s); break;
            case 2: f = gp_tile_sched<2>(A, L, s); break;
            case 3: f = gp_tile_sched<3>(A, L, s); break;
            default: f = gp_tile_sched<4>(A, L, s); break;
        }
        failed = f > failed ? f : failed;
    }
    for (size_t s = 0; s < A.S; s++)
        for (size_t n = 0; n < A.T; n++)
            A.out[n * A.S + s] = gp_tile_sample(A, L, s, (int)(n / kGpTile) * kGpTile, (int)(n % kGpTile), A.window);
    return failed;
}

// the call on host arrays; returns the largest failure code of its streams
static inline int gp_host_render(int mode, const GpArgs &A) {
    int failed = 0;
    for (size_t s = 0; s < A.S; s++) {
        const int f = gp_walk_stream_mode(mode, A, s, A.window);
        failed = f > failed ? f : failed;
    }
    return failed;
}
#endif

}  // namespace
}  // namespace mxg
