// include/maxiReverb.h -- drop-in maxiSatReverb, maxiFreeVerb, maxiFreeVerbStereo and maxiDattaroReverb (the reference's
// src/libs/maxiReverb.h) over mxg_reverb_render (K13) and mxg_dattaro_render (K14): one bank-of-one launch per call, like
// maxiFlanger / maxiChorus in maximilian.h.
//
// Every call uploads its arguments (24 bytes), renders one voice and one sample on the library's stream and reads the one or two
// output samples back.  A fresh object allocates, at its first call, only the ring slots the class ever touches (3 992 / 18 905 /
// 12 587 doubles, at most 151 KB) rather than the reference's 23 MB of 44 100-slot rings.  The objects are value types: a copy
// carries the rings, indices, low-pass states and (w, cut) device-to-device and continues from the same state.  After a device
// failure every call returns silence; nothing throws.  What the reference computes is kept, quirks included (INTEGRATION.md
// section 4): the stereo class's right channel is the allpass chain fed 0.0 on the left channel's rings, and its roomsize /
// absorbtion change nothing.
// maxiDattaroReverb fixes its ten delay lengths from maxiSettings::sampleRate in its constructor, in the reference's float
// arithmetic; a later change of the sample rate does nothing to an existing object, and a copy keeps its source's lengths.  Its
// rings (32 312 doubles at 44 100 Hz) are allocated at the first call.  The reference's 3 100-slot pre-delay ring is not carried:
// its output is used by nothing and no call can observe it.  A sample rate the kernel does not accept (outside 3 345 ..
// 295 129 Hz) prints one line and plays silence.
// maxiReverbFilters, the helper class a patch builds its own reverb from, is a host value type over the per-object part of the
// step header the network kernel K30 shares (maximilian_amd/csrc/mxg_revfilt_obj.h, which must lie beside include/ as it does in
// this tree): no device call per sample.  Banks of many voices of such a network run on the device (maxiReverbNetBank in
// maximilian_bank.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../maximilian_amd/csrc/mxg_revfilt_obj.h"
#include "maximilian.h"

namespace maxigpu {
namespace ps {
struct ReverbLine {
    // one allocation: rings f64 [S] | lp f64 [8] | wc f64 [2] | args f64 [3] = in, roomsize, absorbtion | out f64 [2] | idx i32 [F]
    int kind;
    uint32_t S = 0, F = 0;
    unsigned char *d = nullptr;
    explicit ReverbLine(int k) : kind(k) {}
    size_t bytes() const { return sizeof(double) * (S + 15) + sizeof(int32_t) * F; }
    double *lp() const { return reinterpret_cast<double *>(d) + S; }
    bool init() {
        if (dead()) return false;
        if (d) return true;
        uint32_t nc = 0, na = 0;
        if (!check(mxg_init(-1), "mxg_init") || !check(mxg_reverb_layout_host(kind, &nc, &na, &S, nullptr, nullptr), "mxg_reverb_layout_host"))
            return false;
        F = nc + na;
        d = static_cast<unsigned char *>(mxg_malloc(bytes()));
        if (!d) {
            check(MXG_ERR_HIP, "mxg_malloc (reverb rings)");
            return false;
        }
        const double wc[2] = {0.84, 0.2};  // a fresh maxiFreeVerb's comb weight and low-pass cutoff
        return check(mxg_memset(d, 0, bytes(), nullptr), "mxg_memset") &&
               check(mxg_memcpy_h2d(lp() + 8, wc, sizeof(wc), nullptr), "h2d reverb state") && check(mxg_sync(), "mxg_sync");
    }
    void release() {
        if (d) mxg_free(d);
        d = nullptr;
    }
    void copy_from(const ReverbLine &o) {
        if (!o.d) {  // the source has not played yet: a fresh object again
            release();
            return;
        }
        if (!init()) return;
        check(mxg_memcpy_d2d_async(d, o.d, bytes(), nullptr), "d2d reverb state") && check(mxg_stream_sync(nullptr), "mxg_stream_sync");
    }
    // one sample; out[0], out[1] (the second only for the stereo kind)
    void run(int mode, double x, double room, double absorb, double *out) {
        out[0] = out[1] = 0.0;
        if (!init()) return;
        double *p = lp();
        const double a[3] = {x, room, absorb};
        if (!check(mxg_memcpy_h2d(p + 10, a, sizeof(a), nullptr), "h2d reverb arguments")) return;
        const bool fv = kind == MXG_REVERB_FREEVERB;
        if (!check(mxg_reverb_render(kind, mode, 1, 1, p + 10, p + 11, p + 12, 0, reinterpret_cast<double *>(d),
                                     reinterpret_cast<int32_t *>(p + 15), fv ? p : nullptr, fv ? p + 8 : nullptr, p + 13, nullptr),
                   "mxg_reverb_render"))
            return;
        double o[2] = {0.0, 0.0};
        if (!check(mxg_memcpy_d2h(o, p + 13, sizeof(o), nullptr), "d2h reverb output")) return;
        out[0] = o[0];
        out[1] = kind == MXG_REVERB_FREEVERB_STEREO ? o[1] : 0.0;
    }
};
struct DattaroLine {
    // one allocation: rings f64 [S] | state f64 [5] | in f64 [1] | out f64 [2] | idx i32 [10]
    uint32_t rate;
    uint32_t S = 0;
    unsigned char *d = nullptr;
    DattaroLine() : rate(maxiSettings::sampleRate > 0xffffffffu ? 0xffffffffu : static_cast<uint32_t>(maxiSettings::sampleRate)) {}
    size_t bytes() const { return sizeof(double) * (S + 8) + sizeof(int32_t) * MXG_DATTARO_RINGS; }
    double *state() const { return reinterpret_cast<double *>(d) + S; }
    bool init() {
        if (dead()) return false;
        if (d) return true;
        if (!check(mxg_init(-1), "mxg_init") ||
            !check(mxg_dattaro_layout_host(rate, nullptr, nullptr, &S, nullptr, nullptr), "mxg_dattaro_layout_host"))
            return false;
        d = static_cast<unsigned char *>(mxg_malloc(bytes()));
        if (!d) {
            check(MXG_ERR_HIP, "mxg_malloc (maxiDattaroReverb rings)");
            return false;
        }
        return check(mxg_memset(d, 0, bytes(), nullptr), "mxg_memset") && check(mxg_sync(), "mxg_sync");
    }
    void release() {
        if (d) mxg_free(d);
        d = nullptr;
    }
    void copy_from(const DattaroLine &o) {  // the lengths are the source's, whatever the sample rate is now
        if (!o.d || rate != o.rate) release();
        rate = o.rate;
        if (!o.d || !init()) return;  // (a source that has not played yet: a fresh object again)
        check(mxg_memcpy_d2d_async(d, o.d, bytes(), nullptr), "d2d maxiDattaroReverb state") && check(mxg_stream_sync(nullptr), "mxg_stream_sync");
    }
    void run(double x, double *out) {
        out[0] = out[1] = 0.0;
        if (!init()) return;
        double *p = state();
        if (!check(mxg_memcpy_h2d(p + 5, &x, sizeof(x), nullptr), "h2d maxiDattaroReverb input")) return;
        if (!check(mxg_dattaro_render(rate, 1, 1, p + 5, reinterpret_cast<double *>(d), reinterpret_cast<int32_t *>(p + 8), p, p + 6, nullptr),
                   "mxg_dattaro_render"))
            return;
        double o[2] = {0.0, 0.0};
        if (!check(mxg_memcpy_d2h(o, p + 6, sizeof(o), nullptr), "d2h maxiDattaroReverb output")) return;
        out[0] = o[0];
        out[1] = o[1];
    }
};
}  // namespace ps
}  // namespace maxigpu

#define MAXIGPU_REVERB_VALUE_TYPE(Class, KIND)                       \
    maxigpu::ps::ReverbLine line_{KIND};                             \
    double stereooutput[2] = {0.0, 0.0};                             \
                                                                     \
public:                                                              \
    Class() = default;                                               \
    Class(const Class &o) { line_.copy_from(o.line_); }              \
    Class &operator=(const Class &o) {                               \
        if (this != &o) line_.copy_from(o.line_);                    \
        return *this;                                                \
    }                                                                \
    ~Class() { line_.release(); }

class maxiSatReverb {
    MAXIGPU_REVERB_VALUE_TYPE(maxiSatReverb, MXG_REVERB_SAT)
    double play(double input) {
        line_.run(MXG_REVERB_PLAY, input, 0.0, 0.0, stereooutput);
        return stereooutput[0];
    }
    double *playStereo(double input) {  // {b, -b}
        line_.run(MXG_REVERB_PLAY, input, 0.0, 0.0, stereooutput);
        stereooutput[1] = -stereooutput[0];
        return stereooutput;
    }
};

class maxiFreeVerb {
    MAXIGPU_REVERB_VALUE_TYPE(maxiFreeVerb, MXG_REVERB_FREEVERB)
    double play(double input) {  // the object's current comb weight and cutoff, 4 allpasses
        line_.run(MXG_REVERB_PLAY, input, 0.0, 0.0, stereooutput);
        return stereooutput[0];
    }
    double play(double input, double roomsize, double absorbtion) {  // sets both for good, 31 allpasses
        line_.run(MXG_REVERB_PLAY_PARAMS, input, roomsize, absorbtion, stereooutput);
        return stereooutput[0];
    }
};

class maxiFreeVerbStereo {
    MAXIGPU_REVERB_VALUE_TYPE(maxiFreeVerbStereo, MXG_REVERB_FREEVERB_STEREO)
    double *playStereo(double input, double roomsize, double absorbtion) {  // (the reference reads neither parameter)
        (void)roomsize;
        (void)absorbtion;
        line_.run(MXG_REVERB_PLAY, input, 0.0, 0.0, stereooutput);
        return stereooutput;
    }
};

#undef MAXIGPU_REVERB_VALUE_TYPE

// The reference's 14 public methods with its signatures and its constructor state: a ring of 44 100 zeros, feedback 0.8,
// gain_cof 0.85, index 0.  The object keeps the whole ring, so a size that grows or shrinks mid-stream behaves like the
// reference for as long as the reference stays inside its ring; an index, a tapdpos position or a tap that would leave the
// 44 100 slots reads 0.0 and stores nothing (the reference reads and writes outside its valarray there).  setlength is declared
// by the reference and defined nowhere; here it sets the length that gettap wraps at until the next call sets its own.
class maxiReverbFilters {
public:
    maxiReverbFilters() : delay_line(mxg::RF_RING, 0.0) {}
    double twopoint(double input) { return mxg::rf_obj_twopoint(s, input); }
    double comb1(double input, double size) { return mxg::rf_obj_comb1(s, delay_line.data(), input, size); }
    double combff(double input, double size) { return mxg::rf_obj_combff(s, delay_line.data(), input, size); }
    double combfb(double input, double size, double fb) { return mxg::rf_obj_combfb(s, delay_line.data(), input, size, fb); }
    double lpcombfb(double input, double size, double fb, double cutoff) {
        return mxg::rf_obj_lpcombfb(s, delay_line.data(), input, size, fb, cutoff);
    }
    double allpass(double input, double size) { return mxg::rf_obj_allpass(s, delay_line.data(), input, size, s.gain_cof); }
    double allpass(double input, double size, double fback) { return mxg::rf_obj_allpass(s, delay_line.data(), input, size, fback); }
    double allpasstap(double input, double size, int tap) { return mxg::rf_obj_allpasstap(s, delay_line.data(), input, size, tap); }
    void setlength(int length) { s.delay_size = length; }
    double onetap(double input, double size) { return mxg::rf_obj_onetap(s, delay_line.data(), input, size); }
    double tapd(double input, double size, double *taps, int numtaps) {
        return mxg::rf_obj_tapd(s, delay_line.data(), input, size, taps, numtaps);
    }
    double tapdwgain(double input, double size, double *taps, int numtaps, double *gain) {
        return mxg::rf_obj_tapdwgain(s, delay_line.data(), input, size, taps, numtaps, gain);
    }
    double tapdpos(double input, int size, int *taps, int numtaps) {
        return mxg::rf_obj_tapdpos(s, delay_line.data(), input, size, taps, numtaps);
    }
    double gettap(int tap) { return mxg::rf_obj_gettap(s, delay_line.data(), tap); }

private:
    std::vector<double> delay_line;
    mxg::RfState s;
};

class maxiDattaroReverb {
    maxigpu::ps::DattaroLine line_;  // (captures maxiSettings::sampleRate)
    double stereooutput[2] = {0.0, 0.0};

public:
    maxiDattaroReverb() = default;
    maxiDattaroReverb(const maxiDattaroReverb &o) { line_.copy_from(o.line_); }
    maxiDattaroReverb &operator=(const maxiDattaroReverb &o) {
        if (this != &o) line_.copy_from(o.line_);
        return *this;
    }
    ~maxiDattaroReverb() { line_.release(); }
    double *playStereo(double input) {
        line_.run(input, stereooutput);
        return stereooutput;
    }
};
