// include/maxiPolyBLEP.h -- drop-in for the reference's src/libs/maxiPolyBLEP.h: the anti-aliased oscillator, one sample per call,
// computed on the device (mxg_polyblep_render, K20) through the per-sample engine of maximilian.h.  The slot's state is the phase;
// the waveform is the call's method; frequency, pulse width and sample rate are call arguments, so the engine predicts blocks as
// it does for maxiOsc.  The phase and the ten arithmetic waveforms are the reference's bits, the sine waveforms and the sine
// fallback at freq >= sampleRate / 4 within the bounds of DESIGN.md section 4.  Value semantics: a copy is a second oscillator in
// the same state.
#pragma once
#include <cmath>

#include "maximilian.h"

class maxiPolyBLEP {
    using Pool = maxigpu::ps::PolyBLEPPool;
    maxigpu::ps::Slot slot_;

public:
    enum Waveform {
        SINE, COSINE, TRIANGLE, SQUARE, RECTANGLE, SAWTOOTH, RAMP, MODIFIED_TRIANGLE, MODIFIED_SQUARE, HALF_WAVE_RECTIFIED_SINE,
        FULL_WAVE_RECTIFIED_SINE, TRIANGULAR_PULSE, TRAPEZOID_FIXED, TRAPEZOID_VARIABLE
    };

    maxiPolyBLEP() : sr_((double)maxiSettings::sampleRate) { maxigpu::ps::pool<Pool>().attach(slot_); }
    ~maxiPolyBLEP() { maxigpu::ps::pool<Pool>().detach(slot_); }
    maxiPolyBLEP(const maxiPolyBLEP &o) { maxigpu::ps::pool<Pool>().attach(slot_); copy_from(o); }
    maxiPolyBLEP &operator=(const maxiPolyBLEP &o) { if (this != &o) copy_from(o); return *this; }

    double play(double freq) {  // setFrequency(freq); getAndInc()
        maxigpu::ps::Call c;
        c.method = (int)wf_;
        c.key = Pool::rate_key(sr_);
        c.a[0] = freq; c.a[1] = pw_; c.a[2] = sr_;
        return maxigpu::ps::pool<Pool>().call(slot_, c);
    }
    void setWaveform(Waveform waveform) { maxigpu::ps::pool<Pool>().settle(slot_); wf_ = waveform; }
    void setPulseWidth(double pw) { maxigpu::ps::pool<Pool>().settle(slot_); pw_ = pw; }
    void setSampleRate(double sampleRate) { maxigpu::ps::pool<Pool>().settle(slot_); sr_ = sampleRate; }
    void sync(double phase) {  // PolyBLEP::sync: t = phase - (int64)phase, a negative phase t = phase + (1 - (int64)phase)
        maxigpu::ps::pool<Pool>().settle(slot_);
        slot_.sd[0] = phase >= 0 ? phase - std::trunc(phase) : phase + (1 - std::trunc(phase));
    }

private:
    void copy_from(const maxiPolyBLEP &o) {
        maxigpu::ps::pool<Pool>().settle(const_cast<maxiPolyBLEP &>(o).slot_);
        maxigpu::ps::pool<Pool>().settle(slot_);
        slot_.sd = o.slot_.sd;
        wf_ = o.wf_; pw_ = o.pw_; sr_ = o.sr_;
    }
    Waveform wf_ = SINE;
    double pw_ = 0.5, sr_ = 44100.0;
};
