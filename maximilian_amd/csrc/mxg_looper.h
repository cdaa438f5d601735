// mxg_looper.h -- the members of maxiSample that WRITE the buffer, as plain arithmetic: loopRecord (H:706-721, with the private
// maxiLagExp<double> loopRecordLag of H:523-526 at its default alpha 0.5) and normalise (C:1126-1137), plus the two players that
// a looper slot fuses behind its record head, play() (C:740-747) and playLoop (C:960-967).  C = src/maximilian.cpp, H =
// src/maximilian.h.  No device state: the same text compiles for the host (tests/host_looper.cpp, the mxg_*_host entry points)
// and for the kernels of looper.hip (K25).  Every operation is + - * /, a compare or a cast, never contracted into an FMA, so
// host and device give the reference's bits.
//
// One sample of a slot, in the reference's call order (loopRecord, then the player):
//   lag = (0.5 * enabled) + (0.5 * lag);  if (recpos < start * len) recpos = start * len;
//   enabled:  a[(int)recpos] = (((mix * (a[(int)recpos] / 32767.0)) + ((1.0 - mix) * in)) * lag) * 32767;
//   ++recpos;  if (recpos >= end * len) recpos = start * len;          (whether enabled or not)
//   out = play() or playLoop(pstart, pend) on the same buffer: it sees what this sample and earlier ones recorded.
// The one departure: an index outside [0, len) (start / end outside [0, 1], start == 1, NaN, an uploaded position out of range
// -- the reference indexes outside its vector there) reads 0, stores nothing and is counted (lp_rec_index returns -1; a NaN
// or negative position is never cast).  The players' step is the one of mxg_smp.h (smp_gen<0> / smp_gen<2>), restated here so
// that the host pass of looper.hip can run it too; tests/host_looper.cpp holds the two side by side.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

#define MXG_LOOPER_PLAY_NONE (-1)  // no fused play head; the other two values are MXG_SMP_PLAY (0) and MXG_SMP_PLAYLOOP (2)
#define MXG_LOOPER_MAX_N ((size_t)1 << 24)
#define MXG_LOOPER_MAX_CAP ((size_t)0x7fffff00)  // (int)recordPosition (H:713) must hold every index

namespace mxg {
namespace {

constexpr int kLpPlay = 0, kLpPlayLoop = 2;  // = MXG_SMP_PLAY, MXG_SMP_PLAYLOOP (include/maxigpu.h)

struct LpRec {
    double recpos, lag;  // maxiSample::recordPosition, loopRecordLag.val
};

// H:708-710: the lag takes the enable as 0.0 / 1.0 (alpha 0.5, alphaReciprocal 0.5), then the clamp to the loop's start.
// Returns whether the clamp moved the head.
MXG_HD bool lp_rec_begin(LpRec &s, bool enabled, double start, size_t len) {
    s.lag = (0.5 * (double)enabled) + (0.5 * s.lag);
    const double lo = start * (double)len;
    if (s.recpos < lo) {
        s.recpos = lo;
        return true;
    }
    return false;
}

// The element the head is on: (int)recordPosition inside [0, len), -1 outside (the departure; NaN and negatives included).
MXG_HD long long lp_rec_index(double recpos, size_t len) {
    return (recpos >= 0.0 && recpos < (double)len) ? (long long)recpos : -1;
}

// H:713-716: the element's old content and the input -> the element's new content
MXG_HD double lp_rec_value(double current, double newSample, double recordMix, double lag) {
    const double currentSample = current / 32767.0;
    newSample = (recordMix * currentSample) + ((1.0 - recordMix) * newSample);
    newSample *= lag;
    return newSample * 32767;
}

// H:718-720.  Returns whether the head went back to the loop's start.
MXG_HD bool lp_rec_end(LpRec &s, double start, double end, size_t len) {
    s.recpos += 1.0;
    if (s.recpos >= end * (double)len) {
        s.recpos = start * (double)len;
        return true;
    }
    return false;
}

// (long long)x where x is anything: NaN and what lies below the range give a negative number, as the x86-64 conversion does
MXG_HD long long lp_trunc(double x) { return (long long)fmin(fmax(x, -4.0e18), 4.0e18); }

// mxg_smp.h's smp_safe_head: unchanged on [-2, len + 2], pinned to it otherwise (NaN -> -2): the index stays in the guards
MXG_HD double lp_safe_head(double pos, size_t len) { return fmin(fmax(pos, -2.0), (double)len + 2.0); }

// One call of play() (C:740-747) or playLoop(start, end) (C:960-967): advances `pos`, returns the index read (in [-2, len + 2]).
MXG_HD long long lp_play_step(int mode, double &pos, double start, double end, size_t len) {
    if (mode == kLpPlay) {
        const long long idx = (long long)lp_safe_head(pos, len);
        pos += 1.0;
        if ((size_t)lp_trunc(pos) >= len) pos = 0;
        return idx;
    }
    pos += 1.0;
    const double lo = (double)len * start;
    if (pos < lo) pos = lo;
    if ((double)lp_trunc(pos) >= (double)len * end) pos = lo;
    return (long long)lp_safe_head(pos, len);
}

// ---- normalise (C:1126-1137) ---------------------------------------------------------------------------------------
MXG_HD double lp_norm_max(double maxValue, double a) {  // a NaN element never passes the compare
    const double f = fabs(a);
    return f > maxValue ? f : maxValue;
}
MXG_HD float lp_norm_scale(double maxLevel, double maxValue) { return (float)(maxLevel / maxValue); }  // `float scale`: Inf at maxValue 0
MXG_HD double lp_norm_apply(float scale, double a) { return round((double)scale * a); }

// ---- one piece of one slot, as K25 cuts it (looper.hip) -------------------------------------------------------------------
// A piece is at most a launch's samples of one slot.  Its entries lie `tile` apart (entry n at [n * tile]; the kernel keeps a
// tile of slots side by side in LDS).  lp_plan_slot is the serial part -- the lag, the record head, the play head: nothing in it
// depends on a sample value -- and leaves per sample:
//   lag[n]   the lag's value,
//   idx[n]   the element recorded on, inside [0, len), or -1,
//   link[n]  bit 0: enabled; bit 1: the first visit of its element in the piece; bits 2..: 1 + the NEXT visit of the element (0: none),
//   play[n]  >= 0: the visit (<= n) whose value the play head reads; < 0: -(element + 6), to be read from memory.
// lp_walk_element then takes one element from its content before the piece through all its visits in order.
// The visits of an element are found without a search: between two moves of the head (the clamp, the wrap) the elements are
// consecutive, and every wrap goes back to the same element, so the latest earlier visit is in the current run, the run before it
// or the piece's first run.  The plan checks that structure as it goes (consecutive elements inside a run, equal runs after the
// first); where it fails (only outside the domain the reference is defined on) it searches idx[] backwards instead.
constexpr int kLpLinkEn = 1, kLpLinkHead = 2;

MXG_HD void lp_plan_slot(int N, int tile, size_t len, const double *enable, bool enable_all, double start, double end, int play_mode,
                         double pstart, double pend, LpRec &rec, double &pos, uint32_t &drops, double *lag, int *idx, int *link,
                         int *play) {
    // runs of consecutive elements: the current one, the last complete one that is not the first, and the first
    int curBegin = 0, curFirst = -1, lastIdx = -1;
    int prevBegin = 0, prevFirst = 0, prevLen = -1;
    int firstFirst = 0, firstLen = -1;
    int run = 0;
    bool regular = true, moved = false;
    auto find = [&](int target, int nmax) -> int {  // the latest visit m <= nmax of element target, or -1
        if (target < 0 || nmax < 0) return -1;
        if (regular) {
            int m = -1;
            const int j = target - curFirst;
            if (j >= 0 && curBegin + j <= nmax) m = curBegin + j;
            else if (prevLen >= 0 && target >= prevFirst && target - prevFirst < prevLen) m = prevBegin + (target - prevFirst);
            else if (firstLen >= 0 && target >= firstFirst && target - firstFirst < firstLen) m = target - firstFirst;
            return m;  // (a run that is regular holds no -1, so idx[m] is target: nothing to read back)
        }
        for (int m = nmax; m >= 0; m--)
            if (idx[m * tile] == target) return m;
        return -1;
    };
    for (int n = 0; n < N; n++) {
        const int e = n * tile;
        const bool en = enable ? (enable[e] != 0.0) : enable_all;
        if (lp_rec_begin(rec, en, start, len)) moved = true;
        const int i = (int)lp_rec_index(rec.recpos, len);
        if (i < 0) regular = false;
        if (n == 0) {
            curFirst = i;
        } else if (moved) {  // the run before this sample is complete
            const int done = n - curBegin;
            if (run == 0) {
                firstFirst = curFirst;
                firstLen = done;
            } else {
                if (prevLen >= 0 && (curFirst != prevFirst || done != prevLen)) regular = false;
                prevBegin = curBegin;
                prevFirst = curFirst;
                prevLen = done;
            }
            run++;
            curBegin = n;
            curFirst = i;
        } else if (i != lastIdx + 1) {
            regular = false;
        }
        lastIdx = i;
        idx[e] = i;
        lag[e] = rec.lag;
        int l = 0;
        if (i >= 0) {
            const int pv = find(i, n - 1);
            l = en ? kLpLinkEn : 0;
            if (pv < 0) l |= kLpLinkHead;
            else link[pv * tile] |= (n + 1) << 2;
        } else if (en) {
            drops++;
        }
        link[e] = l;
        moved = lp_rec_end(rec, start, end, len);
        if (play_mode != MXG_LOOPER_PLAY_NONE) {
            const long long pi = lp_play_step(play_mode, pos, pstart, pend, len);
            const int m = (pi >= 0 && (size_t)pi < len) ? find((int)pi, n) : -1;
            play[e] = m >= 0 ? m : -(int)(pi + 6);
        }
    }
}

// val[] holds the input on entry; every visit's entry receives the element's content once that sample is done.  c: the element's
// content before the piece -> after it.  Returns whether a visit recorded (whether c must be stored).
MXG_HD bool lp_walk_element(int n, int tile, double mix, double &c, double *val, const double *lag, const int *link) {
    bool any = false;
    int m = n * tile, l = link[m];
    for (;;) {
        if (l & kLpLinkEn) {
            c = lp_rec_value(c, val[m], mix, lag[m]);
            any = true;
        }
        val[m] = c;
        const int nx = l >> 2;
        if (!nx) break;
        m = (nx - 1) * tile;
        l = link[m];
    }
    return any;
}

// ---- the host pass: sample after sample, slot after slot; what the kernel's pieces must add up to ------------------------
// Arguments as mxg_looprec_render (include/maxigpu.h) on host arrays.  pool points at element 0 of slot 0.
inline void lp_host_render(size_t R, size_t N, double *pool, size_t stride, const uint64_t *len, const double *in, const double *enable,
                           int eps, const double *mix, const double *start, const double *end, double *recpos, double *lagval, int play_mode,
                           const double *pstart, const double *pend, double *position, double *out, uint32_t *dropped) {
    for (size_t r = 0; r < R; r++) {
        double *a = pool + r * stride;
        const size_t L = (size_t)len[r];
        LpRec s = {recpos[r], lagval[r]};
        double pos = play_mode != MXG_LOOPER_PLAY_NONE ? position[r] : 0.0;
        uint32_t drops = 0;
        for (size_t n = 0; n < N; n++) {
            const bool en = enable[eps ? n * R + r : r] != 0.0;
            lp_rec_begin(s, en, start[r], L);
            if (en) {
                const long long i = lp_rec_index(s.recpos, L);
                if (i >= 0) a[i] = lp_rec_value(a[i], in[n * R + r], mix[r], s.lag);
                else drops++;
            }
            lp_rec_end(s, start[r], end[r], L);
            if (play_mode != MXG_LOOPER_PLAY_NONE)
                out[n * R + r] = a[lp_play_step(play_mode, pos, pstart ? pstart[r] : 0.0, pend ? pend[r] : 0.0, L)];
        }
        recpos[r] = s.recpos;
        lagval[r] = s.lag;
        if (play_mode != MXG_LOOPER_PLAY_NONE) position[r] = pos;
        if (dropped) dropped[r] += drops;
    }
}

inline void lp_host_normalise(size_t R, double *pool, size_t stride, const uint64_t *len, const double *maxLevel) {
    for (size_t r = 0; r < R; r++) {
        double *a = pool + r * stride;
        double maxValue = 0;
        for (size_t i = 0; i < (size_t)len[r]; i++) maxValue = lp_norm_max(maxValue, a[i]);
        const float scale = lp_norm_scale(maxLevel[r], maxValue);
        for (size_t i = 0; i < (size_t)len[r]; i++) a[i] = lp_norm_apply(scale, a[i]);
    }
}

}  // namespace
}  // namespace mxg
