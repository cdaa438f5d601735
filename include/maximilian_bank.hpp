// include/maximilian_bank.hpp -- C++ host facade over the C-ABI (include/maxigpu.h).
//
// Host code stays ordinary C++ (g++, no HIP headers): these classes keep the reference's class
// and method names (src/maximilian.h, src/libs/*.h) but stand for a BANK of V instances whose
// state lives in HBM.  Two ways to use a bank:
//
//   block API      bank.sinebuf(N)            -> device block [N][V] (one launch), chain it into
//                                                the next bank (filter, mix ...) without leaving HBM
//   per-sample API bank.frame(v) / bank.tick() -> what the reference's per-sample call returns for
//                                                voice v in the current audio frame; blocks of
//                                                `blockSize` frames are rendered behind the scenes
//                                                when the frame counter wraps, so an existing
//                                                `void play(double *output)` keeps its shape
//                                                (see host/polysynth_host.cpp).
//
// Parameters handed to a bank (frequencies, cutoffs, pans ...) are block-rate: they take effect
// at the next block boundary, the same way the reference's players read control values once
// per callback buffer.  Every method that can fail throws std::runtime_error carrying
// mxg_last_error(); nothing here falls back to the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "maxigpu.h"

namespace maxigpu {

inline void check(int status, const char *what) {
    if (status < 0) throw std::runtime_error(std::string(what) + ": " + mxg_last_error());
}

// RAII device array of T (hipMalloc behind mxg_malloc)
template <typename T>
class DeviceArray {
public:
    DeviceArray() = default;
    explicit DeviceArray(size_t n, bool zero = true) { resize(n, zero); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    DeviceArray(DeviceArray &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceArray &operator=(DeviceArray &&o) noexcept {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DeviceArray() { release(); }
    void resize(size_t n, bool zero = true) {
        release();
        check(mxg_init(-1), "mxg_init");
        p_ = static_cast<T *>(mxg_malloc(n * sizeof(T)));
        if (!p_) throw std::runtime_error(std::string("mxg_malloc: ") + mxg_last_error());
        n_ = n;
        if (zero && n) {  // complete before any launch on any stream can touch the array
            check(mxg_memset(p_, 0, n * sizeof(T), nullptr), "mxg_memset");
            check(mxg_stream_sync(nullptr), "mxg_stream_sync");
        }
    }
    void upload(const T *h, size_t n, size_t offset = 0) {
        check(mxg_memcpy_h2d(p_ + offset, h, n * sizeof(T), nullptr), "mxg_memcpy_h2d");
    }
    void upload(const std::vector<T> &h) {
        if (h.size() > n_) resize(h.size(), false);  // an array that was never sized grows to fit
        upload(h.data(), h.size());
    }
    void download(T *h, size_t n, size_t offset = 0) const {
        check(mxg_memcpy_d2h(h, p_ + offset, n * sizeof(T), nullptr), "mxg_memcpy_d2h");
    }
    std::vector<T> download() const {
        std::vector<T> h(n_);
        if (n_) download(h.data(), n_);
        return h;
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }

private:
    void release() {
        if (p_) mxg_free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace maxigpu

// maxiSettings (H:117-163)
class maxiSettings {
public:
    static size_t sampleRate, channels, bufferSize;
    static void setup(size_t initSampleRate, size_t initChannels, size_t initBufferSize) {
        maxigpu::check(mxg_settings(initSampleRate, initChannels, initBufferSize), "mxg_settings");
        sampleRate = initSampleRate;
        channels = initChannels;
        bufferSize = initBufferSize;
    }
    static size_t getSampleRate() { return sampleRate; }
};
inline size_t maxiSettings::sampleRate = 44100;
inline size_t maxiSettings::channels = 2;
inline size_t maxiSettings::bufferSize = 1024;

namespace maxigpu {

// Common machinery of a bank that produces one [N][V] block per launch and can serve it back
// frame by frame on the host.
class BlockServer {
public:
    BlockServer(size_t voices, size_t blockSize) : V(voices), B(blockSize), out_(voices * blockSize, false) {}
    size_t voices() const { return V; }
    size_t blockSize() const { return B; }
    double *deviceBlock() const { return out_.get(); }

protected:
    // per-sample facade: value of voice v in the current frame; fetches the block on first use
    template <typename RenderFn>
    double frame(size_t v, RenderFn render) {
        if (cursor_ == B || host_.empty()) {
            render(B, out_.get());
            host_.resize(V * B);
            out_.download(host_.data(), V * B);
            cursor_ = 0;
        }
        return host_[cursor_ * V + v];
    }
    void advance() { if (!host_.empty()) ++cursor_; }
    size_t V, B;
    DeviceArray<double> out_;
    std::vector<double> host_;
    size_t cursor_ = 0;
};

}  // namespace maxigpu

// ---- maxiOsc (H:169-215) -------------------------------------------------------------------------
class maxiOscBank : public maxigpu::BlockServer {
public:
    explicit maxiOscBank(size_t voices, size_t blockSize = 512)
        : BlockServer(voices, blockSize), freq_(voices), p1_(voices), p2_(voices), phase_(voices), hold_(voices) {}
    void setFrequencies(const std::vector<double> &f) { freq_.upload(f); }
    void setDuty(const std::vector<double> &d) { p1_.upload(d); }
    void setPhasorRange(const std::vector<double> &start, const std::vector<double> &end) { p1_.upload(start); p2_.upload(end); }
    void phaseReset(const std::vector<double> &phaseIn) { phase_.upload(phaseIn); }  // C:222-226
    std::vector<double> phases() const { return phase_.download(); }

    // block API: N samples of every voice into d_out ([N][V], device), state carried
    void render(int waveform, size_t N, double *d_out, const double *d_freq_per_sample = nullptr, void *stream = nullptr) {
        maxigpu::check(mxg_osc_render(waveform, V, N, d_freq_per_sample ? d_freq_per_sample : freq_.get(),
                                      d_freq_per_sample ? 1 : 0, p1_.get(), p2_.get(), phase_.get(), hold_.get(),
                                      d_out, stream), "mxg_osc_render");
    }
    void sinewave(size_t N, double *d_out) { render(MXG_OSC_SINEWAVE, N, d_out); }
    void coswave(size_t N, double *d_out) { render(MXG_OSC_COSWAVE, N, d_out); }
    void phasor(size_t N, double *d_out) { render(MXG_OSC_PHASOR, N, d_out); }
    void saw(size_t N, double *d_out) { render(MXG_OSC_SAW, N, d_out); }
    void triangle(size_t N, double *d_out) { render(MXG_OSC_TRIANGLE, N, d_out); }
    void square(size_t N, double *d_out) { render(MXG_OSC_SQUARE, N, d_out); }
    void pulse(size_t N, double *d_out) { render(MXG_OSC_PULSE, N, d_out); }
    void impulse(size_t N, double *d_out) { render(MXG_OSC_IMPULSE, N, d_out); }
    void sinebuf(size_t N, double *d_out) { render(MXG_OSC_SINEBUF, N, d_out); }
    void sinebuf4(size_t N, double *d_out) { render(MXG_OSC_SINEBUF4, N, d_out); }
    void sawn(size_t N, double *d_out) { render(MXG_OSC_SAWN, N, d_out); }
    void phasorBetween(size_t N, double *d_out) { render(MXG_OSC_PHASORBETWEEN, N, d_out); }
    // noise() (C:214-220): d_rand = the rand() draws, int32 [N][V] (draw n*V+v for a voice-inner loop)
    void noise(size_t N, const int32_t *d_rand, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_osc_noise(V, N, d_rand, hold_.get(), d_out, stream), "mxg_osc_noise");
    }

    // per-sample API: `waveform` is fixed for the facade stream; call tick() once per audio frame
    void setWaveform(int waveform) { waveform_ = waveform; }
    double frame(size_t v) {
        return BlockServer::frame(v, [this](size_t N, double *d) { render(waveform_, N, d); });
    }
    void tick() { advance(); }

private:
    maxigpu::DeviceArray<double> freq_, p1_, p2_, phase_, hold_;
    int waveform_ = MXG_OSC_SINEBUF;
};

// ---- maxiFilter (H:289-366) ------------------------------------------------------------------------
class maxiFilterBank {
public:
    explicit maxiFilterBank(size_t voices) : V(voices), state_(5 * voices), cutoff_(voices), res_(voices), coef_(3 * voices) {}
    // block-constant parameters: coefficients on the host libm (bit-exact recurrence)
    void setParams(int kind, const std::vector<double> &cutoff, const std::vector<double> &resonance) {
        cutoff_.upload(cutoff);
        if (kind <= MXG_FLT_BANDPASS) {
            res_.upload(resonance);
            std::vector<double> coef(3 * V);
            maxigpu::check(mxg_filter_coeffs_host(kind, V, cutoff.data(), resonance.data(), coef.data()), "mxg_filter_coeffs_host");
            coef_.upload(coef);
        }
        kind_ = kind;
    }
    void render(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_filter_render(kind_, V, N, d_in, cutoff_.get(), 0, res_.get(), 0, coef_.get(), state_.get(),
                                         d_out, stream), "mxg_filter_render");
    }
    // audio-rate modulated cutoff ([N][V] on device), device coefficients, stated tolerance
    void renderModulated(int kind, size_t N, const double *d_in, const double *d_cutoff, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_filter_render(kind, V, N, d_in, d_cutoff, 1, res_.get(), 0, nullptr, state_.get(), d_out, stream),
                       "mxg_filter_render");
    }
    std::vector<double> state() const { return state_.download(); }

private:
    size_t V;
    int kind_ = MXG_FLT_LORES;
    maxigpu::DeviceArray<double> state_, cutoff_, res_, coef_;
};

// ---- maxiDCBlocker / maxiSVF / maxiBiquad (H:1255-1486) --------------------------------------------------
class maxiDCBlockerBank {
public:
    explicit maxiDCBlockerBank(size_t voices) : V(voices), state_(3 * voices), R_(voices) {}
    void setR(const std::vector<double> &R) { R_.upload(R); }
    void play(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {  // play(input, R) H:1261-1266
        maxigpu::check(mxg_filter2_render(0, V, N, d_in, R_.get(), state_.get(), d_out, stream), "mxg_filter2_render");
    }

private:
    size_t V;
    maxigpu::DeviceArray<double> state_, R_;
};

class maxiSVFBank {
public:
    explicit maxiSVFBank(size_t voices) : V(voices), freq_(voices, 1000.0), res_(voices, 1.0), mix_(4 * voices, 0.0), state_(3 * voices), coef_(9 * voices) {}
    void setCutoff(const std::vector<double> &cutoff) { freq_ = cutoff; dirty_ = true; }   // H:1287-1290
    void setResonance(const std::vector<double> &q) { res_ = q; dirty_ = true; }          // H:1293-1296
    void setMix(double lpmix, double bpmix, double hpmix, double notchmix) {              // the play() arguments
        for (size_t v = 0; v < V; v++) { mix_[v] = lpmix; mix_[V + v] = bpmix; mix_[2 * V + v] = hpmix; mix_[3 * V + v] = notchmix; }
        dirty_ = true;
    }
    void play(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {      // H:1303-1317
        if (dirty_) {
            std::vector<double> c(9 * V);
            maxigpu::check(mxg_svf_coeffs_host(V, freq_.data(), res_.data(), c.data()), "mxg_svf_coeffs_host");
            std::copy(mix_.begin(), mix_.end(), c.begin() + 5 * V);
            coef_.upload(c);
            dirty_ = false;
        }
        maxigpu::check(mxg_filter2_render(1, V, N, d_in, coef_.get(), state_.get(), d_out, stream), "mxg_filter2_render");
    }

private:
    size_t V;
    std::vector<double> freq_, res_, mix_;
    maxigpu::DeviceArray<double> state_, coef_;
    bool dirty_ = true;
};

class maxiBiquadBank {
public:
    enum filterTypes { LOWPASS, HIGHPASS, BANDPASS, NOTCH, PEAK, LOWSHELF, HIGHSHELF };
    explicit maxiBiquadBank(size_t voices) : V(voices), state_(3 * voices), coef_(5 * voices) {}
    void set(filterTypes filtType, const std::vector<double> &cutoff, const std::vector<double> &Q, const std::vector<double> &peakGain) {  // H:1376-1478
        std::vector<int32_t> t(V, (int32_t)filtType);
        std::vector<double> c(5 * V);
        maxigpu::check(mxg_biquad_coeffs_host(V, t.data(), cutoff.data(), Q.data(), peakGain.data(), c.data()), "mxg_biquad_coeffs_host");
        coef_.upload(c);
    }
    void play(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {  // H:1360-1367
        maxigpu::check(mxg_filter2_render(2, V, N, d_in, coef_.get(), state_.get(), d_out, stream), "mxg_filter2_render");
    }

private:
    size_t V;
    maxigpu::DeviceArray<double> state_, coef_;
};

// ---- maxiEnv (H:888-932) ------------------------------------------------------------------------------
class maxiEnvBank {
public:
    explicit maxiEnvBank(size_t voices)
        : V(voices), par_h_(4 * voices, 0.0), hold_h_(voices, 1), par_(4 * voices), hold_(voices), dst_(2 * voices), ist_(6 * voices) {}
    void setAttack(double ms) { fill(0, mxg_env_coeff_host(0, ms)); }      // C:1480-1482
    void setAttackMS(double ms) { fill(0, mxg_env_coeff_host(3, ms)); }    // C:1486-1488
    void setDecay(double ms) { fill(1, mxg_env_coeff_host(1, ms)); }       // C:1475-1477
    void setSustain(double level) { fill(2, level); }                     // C:1492-1494
    void setRelease(double ms) { fill(3, mxg_env_coeff_host(2, ms)); }     // C:1470-1472
    void setHoldtime(long holdtime) { for (auto &h : hold_h_) h = holdtime; dirty_ = true; }
    // trigger: int32 [N] on device (shared gate) or [N][V] (per voice)
    void adsr(size_t N, const double *d_in, const int32_t *d_trig, bool per_voice, double *d_out, void *stream = nullptr) {
        sync();
        maxigpu::check(mxg_env_render(0, V, N, d_in, d_trig, per_voice ? 1 : 0, par_.get(), hold_.get(), dst_.get(), ist_.get(),
                                      d_out, stream), "mxg_env_render");
    }
    void ar(size_t N, const double *d_in, const int32_t *d_trig, bool per_voice, double *d_out, void *stream = nullptr) {
        sync();
        maxigpu::check(mxg_env_render(1, V, N, d_in, d_trig, per_voice ? 1 : 0, par_.get(), hold_.get(), dst_.get(), ist_.get(),
                                      d_out, stream), "mxg_env_render");
    }
    const double *params() { sync(); return par_.get(); }
    const int64_t *holdtimes() { sync(); return hold_.get(); }
    double *dstate() { return dst_.get(); }
    int64_t *istate() { return ist_.get(); }

private:
    void fill(int row, double v) { for (size_t i = 0; i < V; i++) par_h_[row * V + i] = v; dirty_ = true; }
    void sync() { if (dirty_) { par_.upload(par_h_); hold_.upload(hold_h_); dirty_ = false; } }
    size_t V;
    std::vector<double> par_h_;
    std::vector<int64_t> hold_h_;
    maxigpu::DeviceArray<double> par_;
    maxigpu::DeviceArray<int64_t> hold_;
    maxigpu::DeviceArray<double> dst_;
    maxigpu::DeviceArray<int64_t> ist_;
    bool dirty_ = true;
};

// ---- maxiEnvGen (H:2268-2547): one envelope shape per bank, per-voice or shared trigger signals --------------
class maxiEnvGenBank {
public:
    static constexpr double HOLD = -46692;  // maxiEnvGen::HOLD
    explicit maxiEnvGenBank(size_t voices) : V(voices), dst_(5 * voices), ist_(7 * voices) { arm(); }
    bool setup(const std::vector<double> &levels, const std::vector<double> &times, const std::vector<double> &curves,
               bool looping, bool allowRetrigger = false) {  // H:2366-2399
        if (!(levels.size() == times.size() + 1 && levels.size() == curves.size() + 1)) return false;
        std::vector<double> st(6 * times.size());
        const int n = mxg_envgen_stages_host(levels.size(), levels.data(), times.data(), curves.data(), st.data());
        if (n < 0) return false;
        stages_.resize(st.size(), false);
        stages_.upload(st);
        nstages_ = n; loop_ = looping; retrigger_ = allowRetrigger;
        arm();
        return true;
    }
    void setupAR(double attack, double release) { setup({0, 1, 0}, {attack, release}, {1, 1}, false, false); }
    void setupASR(double attack, double release) { setup({0, 1, 1, 0}, {attack, HOLD, release}, {1, 1, 1}, false, false); }
    void setupADSR(double attack, double decay, double sustain, double release) {
        setup({0, 1, sustain, sustain, 0}, {attack, decay, HOLD, release}, {1, 1, 1, 1}, false, false);
    }
    void setRetrigger(bool v) { retrigger_ = v; }
    void setLoop(bool v) { loop_ = v; }
    // d_trig: [N][V] (per_voice) or [N] (shared gate), doubles on the device
    void play(size_t N, const double *d_trig, bool per_voice, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_envgen_render(V, N, d_trig, per_voice ? 1 : 0, stages_.get(), nstages_, loop_ ? 1 : 0, retrigger_ ? 1 : 0,
                                         dst_.get(), ist_.get(), d_out, stream), "mxg_envgen_render");
    }

private:
    void arm() {  // resetAndArm() of fresh objects: WAITING, detectors previousValue = 1 / firstTrigger = 1
        std::vector<double> d(5 * V, 0.0);
        std::vector<int64_t> i(7 * V, 0);
        for (size_t v = 0; v < V; v++) { d[2 * V + v] = d[3 * V + v] = d[4 * V + v] = 1.0; i[4 * V + v] = i[5 * V + v] = i[6 * V + v] = 1; }
        dst_.upload(d); ist_.upload(i);
    }
    size_t V;
    int nstages_ = 0;
    bool loop_ = false, retrigger_ = false;
    maxigpu::DeviceArray<double> stages_, dst_;
    maxigpu::DeviceArray<int64_t> ist_;
};

// ---- fused subtractive voice: maxiOsc::saw -> maxiFilter::lores -> maxiEnv::adsr -----------------------
class maxiVoiceBank : public maxigpu::BlockServer {
public:
    explicit maxiVoiceBank(size_t voices, size_t blockSize = 512)
        : BlockServer(voices, blockSize), env(voices), freq_(voices), cutoff_(voices), res_(voices), coef_(3 * voices),
          ost_(2 * voices), fst_(5 * voices), trig_(blockSize) {}
    maxiEnvBank env;
    void setVoices(const std::vector<double> &freq, const std::vector<double> &cutoff, const std::vector<double> &resonance) {
        freq_.upload(freq);
        cutoff_.upload(cutoff);
        res_.upload(resonance);
        std::vector<double> coef(3 * V);
        maxigpu::check(mxg_filter_coeffs_host(MXG_FLT_LORES, V, cutoff.data(), resonance.data(), coef.data()), "mxg_filter_coeffs_host");
        coef_.upload(coef);
    }
    // mode 0: coefficients hoisted (bit-exact); mode 1: cutoff = envelope*cutoff per sample (14.monosynth)
    void render(int mode, size_t N, const int32_t *d_trig, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_voice_render(mode, V, N, freq_.get(), cutoff_.get(), res_.get(), coef_.get(), d_trig, 0, env.params(),
                                        env.holdtimes(), ost_.get(), fst_.get(), env.dstate(), env.istate(), d_out, stream),
                       "mxg_voice_render");
    }
    // The same block with the maxiMix::stereo mixdown of the bank fused into the render (round 6: mxg_voice_render_mix) -- what the user
    // code of 15.polysynth/main.cpp:54-70 computes voice after voice (`mymix.stereo(out, outputs, pan)` + the sums), here as d_mix [N][2]
    // from ONE kernel that never re-reads the block.  d_out may be nullptr (mix only).  setPan() first.
    void setPan(const std::vector<double> &x) { pan_.upload(x); }
    void renderMix(int mode, size_t N, const int32_t *d_trig, double *d_out, double *d_mix, void *stream = nullptr) {
        maxigpu::check(mxg_voice_render_mix(mode, V, N, freq_.get(), cutoff_.get(), res_.get(), coef_.get(), d_trig, 0, env.params(),
                                            env.holdtimes(), ost_.get(), fst_.get(), env.dstate(), env.istate(), d_out, pan_.get(), d_mix,
                                            stream), "mxg_voice_render_mix");
    }
    // per-sample API: the gate for the NEXT block is whatever setGate() holds when the block is rendered
    void setGate(const std::vector<int32_t> &gateForBlock) { trig_.upload(gateForBlock); }
    double frame(size_t v) {
        return BlockServer::frame(v, [this](size_t N, double *d) { render(0, N, trig_.get(), d); });
    }
    // per-sample API of the mixed bank: channel ch (0 / 1) of the current frame's stereo mix, formed on the device
    double mixFrame(int ch) {
        if (mcursor_ == B || mix_host_.empty()) {
            if (mix_.size() < 2 * B) mix_.resize(2 * B, false);
            renderMix(0, B, trig_.get(), nullptr, mix_.get());
            mix_host_.resize(2 * B);
            mix_.download(mix_host_.data(), 2 * B);
            mcursor_ = 0;
        }
        return mix_host_[mcursor_ * 2 + ch];
    }
    void tick() {
        advance();
        if (!mix_host_.empty()) ++mcursor_;
    }

private:
    maxigpu::DeviceArray<double> freq_, cutoff_, res_, coef_, ost_, fst_;
    maxigpu::DeviceArray<int32_t> trig_;
    maxigpu::DeviceArray<double> pan_, mix_;
    std::vector<double> mix_host_;
    size_t mcursor_ = 0;
};

// ---- maxiMix::stereo over a bank + mixdown over voices (C:503-509) ---------------------------------------
class maxiMixBank {
public:
    explicit maxiMixBank(size_t voices) : V(voices), pan_(voices), y_(voices), z_(voices) {}
    void setPan(const std::vector<double> &x) { pan_.upload(x); }
    void setPan(const std::vector<double> &x, const std::vector<double> &y) { pan_.upload(x); y_.upload(y); }
    void setPan(const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &z) {
        pan_.upload(x); y_.upload(y); z_.upload(z);
    }
    // d_mix: [N][2] on device
    void stereo(size_t N, const double *d_in, double *d_mix, void *stream = nullptr) {
        maxigpu::check(mxg_mix_stereo(V, N, d_in, pan_.get(), d_mix, stream), "mxg_mix_stereo");
    }
    // quad (C:512-522): d_mix [N][4]; ambisonic (C:525-541): d_mix [N][8].  d_bus (optional, [N][C][V]) receives
    // the per-voice four/eight signals.
    void quad(size_t N, const double *d_in, double *d_mix, double *d_bus = nullptr, void *stream = nullptr) {
        maxigpu::check(mxg_mix_bus(4, V, N, d_in, pan_.get(), y_.get(), nullptr, d_bus, d_mix, stream), "mxg_mix_bus");
    }
    void ambisonic(size_t N, const double *d_in, double *d_mix, double *d_bus = nullptr, void *stream = nullptr) {
        maxigpu::check(mxg_mix_bus(8, V, N, d_in, pan_.get(), y_.get(), z_.get(), d_bus, d_mix, stream), "mxg_mix_bus");
    }

private:
    size_t V;
    maxigpu::DeviceArray<double> pan_, y_, z_;
};

// ---- maxiDelayline (H:266-284) ---------------------------------------------------------------------------
class maxiDelaylineBank {
public:
    maxiDelaylineBank(size_t voices, size_t capacity)
        : V(voices), cap(capacity), mem_(voices * capacity), phase_(voices), size_(voices), fb_(voices), pos_(voices) {}
    void setParams(const std::vector<int32_t> &size, const std::vector<double> &feedback) { size_.upload(size); fb_.upload(feedback); }
    void setPositions(const std::vector<int32_t> &position) { pos_.upload(position); }
    void dl(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_delay_render(0, V, N, d_in, size_.get(), fb_.get(), nullptr, mem_.get(), cap, phase_.get(), d_out, stream),
                       "mxg_delay_render");
    }
    void dlFromPosition(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_delay_render(1, V, N, d_in, size_.get(), fb_.get(), pos_.get(), mem_.get(), cap, phase_.get(), d_out, stream),
                       "mxg_delay_render");
    }

private:
    size_t V, cap;
    maxigpu::DeviceArray<double> mem_;
    maxigpu::DeviceArray<int32_t> phase_, size_;
    maxigpu::DeviceArray<double> fb_;
    maxigpu::DeviceArray<int32_t> pos_;
};

// ---- maxiFlanger (H:1144-1172) / maxiChorus (H:1179-1212) banks: block-rate parameters per voice --------------------------
// (per-sample parameters: call mxg_flanger_render / mxg_chorus_render with ps_flags).  Rings voice-major, `capacity` slots each;
// a tap above it is held there and counted in overflow() (the reference indexes past its own ring there).
class maxiFlangerBank {
public:
    maxiFlangerBank(size_t voices, size_t capacity)
        : V(voices), cap(capacity), mem_(voices * capacity), phase_(voices), lfo_(voices), ovf_(voices), delay_(voices),
          fb_(voices), speed_(voices), depth_(voices) {}
    void setParams(const std::vector<uint32_t> &delay, const std::vector<double> &feedback, const std::vector<double> &speed,
                   const std::vector<double> &depth) {
        delay_.upload(delay); fb_.upload(feedback); speed_.upload(speed); depth_.upload(depth);
    }
    void flange(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_flanger_render(V, N, d_in, delay_.get(), fb_.get(), speed_.get(), depth_.get(), 0, mem_.get(), cap,
                                          phase_.get(), lfo_.get(), ovf_.get(), d_out, stream), "mxg_flanger_render");
    }
    uint32_t *overflow() { return ovf_.get(); }  // device [V]

private:
    size_t V, cap;
    maxigpu::DeviceArray<double> mem_;
    maxigpu::DeviceArray<int32_t> phase_;
    maxigpu::DeviceArray<double> lfo_;
    maxigpu::DeviceArray<uint32_t> ovf_, delay_;
    maxigpu::DeviceArray<double> fb_, speed_, depth_;
};

class maxiChorusBank {
public:
    maxiChorusBank(size_t voices, size_t capacity)
        : V(voices), cap(capacity), mem_(2 * voices * capacity), phase_(2 * voices), lp_(2 * voices), ovf_(voices),
          delay_(voices), fb_(voices), depth_(voices), coef_(2 * voices) {}
    // speed: the lores cutoff (resonance 1); its coefficients are evaluated here with the host libm
    void setParams(const std::vector<uint32_t> &delay, const std::vector<double> &feedback, const std::vector<double> &speed,
                   const std::vector<double> &depth) {
        delay_.upload(delay); fb_.upload(feedback); depth_.upload(depth);
        std::vector<double> res(V, 1.0), coef(3 * V);
        maxigpu::check(mxg_filter_coeffs_host(MXG_FLT_LORES, V, speed.data(), res.data(), coef.data()), "mxg_filter_coeffs_host");
        coef.resize(2 * V);
        coef_.upload(coef);
    }
    // d_rand: int32 [N][V], the rand() draw each voice's lfo.noise() takes
    void chorus(size_t N, const double *d_in, const int32_t *d_rand, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_chorus_render(V, N, d_in, delay_.get(), fb_.get(), depth_.get(), 0, d_rand, coef_.get(), 0, mem_.get(),
                                         cap, phase_.get(), lp_.get(), ovf_.get(), d_out, stream), "mxg_chorus_render");
    }
    uint32_t *overflow() { return ovf_.get(); }  // device [V]

private:
    size_t V, cap;
    maxigpu::DeviceArray<double> mem_;
    maxigpu::DeviceArray<int32_t> phase_;
    maxigpu::DeviceArray<double> lp_;
    maxigpu::DeviceArray<uint32_t> ovf_, delay_;
    maxigpu::DeviceArray<double> fb_, depth_, coef_;
};

// ---- maxiSatReverb / maxiFreeVerb / maxiFreeVerbStereo banks (libs/maxiReverb.h, K13) --------------------------------------
// Every delay length is a constant of the class; the state sizes come from mxg_reverb_layout_host.  Rings voice-major,
// zeroed like the constructors.  Bit-exact, quirks of the reference included.
class maxiReverbBankBase {
public:
    uint32_t combs() const { return nc_; }
    uint32_t allpasses() const { return na_; }
    uint32_t ringDoubles() const { return S_; }  // per voice
    double *rings() { return rings_.get(); }     // device [V][ringDoubles()]
    int32_t *indices() { return idx_.get(); }    // device [V][combs() + allpasses()]

protected:
    maxiReverbBankBase(int kind, size_t voices)
        : kind_(kind), V(voices), nc_(layout(kind, 0)), na_(layout(kind, 1)), S_(layout(kind, 2)), rings_(voices * S_),
          idx_(voices * (nc_ + na_)) {}
    void render(int mode, size_t N, const double *d_in, const double *d_room, const double *d_absorb, double *d_lp, double *d_wc,
                double *d_out, void *stream) {
        maxigpu::check(mxg_reverb_render(kind_, mode, V, N, d_in, d_room, d_absorb, 0, rings_.get(), idx_.get(), d_lp, d_wc, d_out,
                                         stream), "mxg_reverb_render");
    }
    int kind_;
    size_t V;

private:
    static uint32_t layout(int kind, int which) {
        uint32_t a[3] = {0, 0, 0};
        maxigpu::check(mxg_reverb_layout_host(kind, &a[0], &a[1], &a[2], nullptr, nullptr), "mxg_reverb_layout_host");
        return a[which];
    }
    uint32_t nc_, na_, S_;
    maxigpu::DeviceArray<double> rings_;
    maxigpu::DeviceArray<int32_t> idx_;
};

class maxiSatReverbBank : public maxiReverbBankBase {
public:
    explicit maxiSatReverbBank(size_t voices) : maxiReverbBankBase(MXG_REVERB_SAT, voices) {}
    void play(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        render(MXG_REVERB_PLAY, N, d_in, nullptr, nullptr, nullptr, nullptr, d_out, stream);
    }
};

class maxiFreeVerbBank : public maxiReverbBankBase {
public:
    explicit maxiFreeVerbBank(size_t voices)
        : maxiReverbBankBase(MXG_REVERB_FREEVERB, voices), lp_(voices * 8), wc_(voices * 2), room_(voices), absorb_(voices) {
        std::vector<double> wc(voices * 2);
        for (size_t v = 0; v < voices; v++) {
            wc[2 * v] = 0.84;  // a fresh object's comb weight and low-pass cutoff
            wc[2 * v + 1] = 0.2;
        }
        wc_.upload(wc);
    }
    // play(x): the comb weight and cutoff as they stand, 4 allpasses
    void play(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        render(MXG_REVERB_PLAY, N, d_in, nullptr, nullptr, lp_.get(), wc_.get(), d_out, stream);
    }
    // play(x, roomsize, absorbtion), one value per voice: sets both for good, 31 allpasses
    void play(size_t N, const double *d_in, const std::vector<double> &roomsize, const std::vector<double> &absorbtion, double *d_out,
              void *stream = nullptr) {
        room_.upload(roomsize);
        absorb_.upload(absorbtion);
        render(MXG_REVERB_PLAY_PARAMS, N, d_in, room_.get(), absorb_.get(), lp_.get(), wc_.get(), d_out, stream);
    }
    double *weightAndCutoff() { return wc_.get(); }  // device [V][2]

private:
    maxigpu::DeviceArray<double> lp_, wc_, room_, absorb_;
};

class maxiFreeVerbStereoBank : public maxiReverbBankBase {
public:
    explicit maxiFreeVerbStereoBank(size_t voices) : maxiReverbBankBase(MXG_REVERB_FREEVERB_STEREO, voices) {}
    // d_out [2][N][V]: left, right (the reference's roomsize / absorbtion change nothing and are not taken)
    void playStereo(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        render(MXG_REVERB_PLAY, N, d_in, nullptr, nullptr, nullptr, nullptr, d_out, stream);
    }
};

// ---- maxiDattaroReverb bank (libs/maxiReverb.h, K14) -------------------------------------------------------------------------
// Every delay length is fixed from `sampleRate` at construction, in the reference's float arithmetic (mxg_dattaro_layout_host;
// a rate it does not accept throws).  Rings voice-major, everything zeroed like the constructor.  The reference's unobservable
// pre-delay ring is not carried.  Bit-exact, quirks of the reference included.
class maxiDattaroReverbBank {
public:
    explicit maxiDattaroReverbBank(size_t voices, uint32_t sampleRate = 44100)
        : V(voices), rate_(sampleRate), lay_(sampleRate), rings_(voices * lay_.S), idx_(voices * MXG_DATTARO_RINGS),
          state_(voices * MXG_DATTARO_STATE) {}
    // d_in [N][V]; d_out [2][N][V]: left, right
    void playStereo(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_dattaro_render(rate_, V, N, d_in, rings_.get(), idx_.get(), state_.get(), d_out, stream), "mxg_dattaro_render");
    }
    uint32_t sampleRate() const { return rate_; }
    uint32_t ringDoubles() const { return lay_.S; }                    // per voice
    const uint32_t *lengths() const { return lay_.len; }               // [10]: AP0 AP1 AP4 AP5 AP6 AP7 D0 D1 D2 D3
    const uint32_t *offsets() const { return lay_.off; }               // [10]
    const uint32_t *tapPositions() const { return lay_.tap; }          // [14]
    const uint32_t *tapRings() const { return lay_.tapRing; }          // [14]
    double *rings() { return rings_.get(); }                           // device [V][ringDoubles()]
    int32_t *indices() { return idx_.get(); }                          // device [V][10]
    double *state() { return state_.get(); }                           // device [V][5] = lp0 lp1 lp2 sigl sigr

private:
    struct Layout {
        uint32_t len[MXG_DATTARO_RINGS], off[MXG_DATTARO_RINGS], tap[MXG_DATTARO_TAPS], tapRing[MXG_DATTARO_TAPS], S = 0;
        explicit Layout(uint32_t rate) { maxigpu::check(mxg_dattaro_layout_host(rate, len, off, &S, tap, tapRing), "mxg_dattaro_layout_host"); }
    };
    size_t V;
    uint32_t rate_;
    Layout lay_;
    maxigpu::DeviceArray<double> rings_;
    maxigpu::DeviceArray<int32_t> idx_;
    maxigpu::DeviceArray<double> state_;
};

// ---- custom reverb networks out of maxiReverbFilters stages (libs/maxiReverb.h:42-73, K30) ----------------------------------
// One topology per bank: the parallel combs `combSizes` summed in order -- combfb, or lpcombfb where `combLowpass` flags it
// (empty: every comb plain) -- into the serial allpasses `apSizes`.  Lengths are whole samples in [1, 44100], at most 32 of each
// kind, a low-pass comb at least 64 (mxg_revnet_layout_host; a topology it does not accept throws).  Feedbacks and cutoffs are
// per voice and stage, constant within a call; nothing clamps them.  Rings voice-major, everything zeroed like fresh objects.
class maxiReverbNetBank {
public:
    maxiReverbNetBank(size_t voices, const std::vector<uint32_t> &combSizes, const std::vector<uint32_t> &apSizes,
                      const std::vector<uint32_t> &combLowpass = {}, double combFb = 0.85, double combCut = 0.2, double apFb = 0.85)
        : V(voices), lay_(combSizes, apSizes, combLowpass), rings_(voices * lay_.S), idx_(voices * lay_.F() + 1), lp_(voices * lay_.P() + 1),
          cfb_(voices * lay_.P() + 1), cut_(voices * lay_.P() + 1), afb_(voices * lay_.A() + 1) {
        setCombFb(combFb);
        setCombCut(combCut);
        setApFb(apFb);
    }
    // d_in, d_out [N][V]
    void play(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_revnet_render((uint32_t)lay_.P(), (uint32_t)lay_.A(), lay_.combs.data(), lay_.aps.data(), lay_.lowp.data(), V, N, d_in,
                                         cfb_.get(), cut_.get(), afb_.get(), rings_.get(), idx_.get(), lp_.get(), d_out, stream),
                       "mxg_revnet_render");
    }
    // one value for every voice and stage, or host values [V][stages]; call between blocks (the call waits for the device)
    void setCombFb(double fb) { fill(cfb_, lay_.P(), fb); }
    void setCombCut(double cutoff) { fill(cut_, lay_.P(), cutoff); }
    void setApFb(double fb) { fill(afb_, lay_.A(), fb); }
    void setCombFb(const std::vector<double> &fb) { put(cfb_, lay_.P(), fb); }
    void setCombCut(const std::vector<double> &cutoff) { put(cut_, lay_.P(), cutoff); }
    void setApFb(const std::vector<double> &fb) { put(afb_, lay_.A(), fb); }
    void clear() {  // fresh objects again; the parameters stay
        maxigpu::check(mxg_sync(), "mxg_sync");
        maxigpu::check(mxg_memset(rings_.get(), 0, rings_.size() * sizeof(double), nullptr), "mxg_memset");
        maxigpu::check(mxg_memset(idx_.get(), 0, idx_.size() * sizeof(int32_t), nullptr), "mxg_memset");
        maxigpu::check(mxg_memset(lp_.get(), 0, lp_.size() * sizeof(double), nullptr), "mxg_memset");
        maxigpu::check(mxg_stream_sync(nullptr), "mxg_stream_sync");
    }
    size_t combs() const { return lay_.P(); }
    size_t allpasses() const { return lay_.A(); }
    uint32_t ringDoubles() const { return lay_.S; }                     // per voice
    const std::vector<uint32_t> &offsets() const { return lay_.off; }   // [combs + allpasses], combs first
    double *rings() { return rings_.get(); }                            // device [V][ringDoubles()]
    int32_t *indices() { return idx_.get(); }                           // device [V][combs + allpasses]
    double *lowpassStates() { return lp_.get(); }                       // device [V][combs]
    double *combFb() { return cfb_.get(); }                             // device [V][combs]
    double *combCut() { return cut_.get(); }                            // device [V][combs]
    double *apFb() { return afb_.get(); }                               // device [V][allpasses]

private:
    struct Layout {
        std::vector<uint32_t> combs, aps, lowp, off;
        uint32_t S = 0;
        Layout(const std::vector<uint32_t> &c, const std::vector<uint32_t> &a, const std::vector<uint32_t> &l) : combs(c), aps(a), lowp(l) {
            if (lowp.empty()) lowp.assign(combs.size(), 0);
            if (lowp.size() != combs.size()) throw std::runtime_error("maxiReverbNetBank: one low-pass flag per comb");
            off.assign(combs.size() + aps.size() + 1, 0);
            maxigpu::check(mxg_revnet_layout_host((uint32_t)combs.size(), (uint32_t)aps.size(), combs.data(), aps.data(), lowp.data(),
                                                  combs.size() + aps.size() <= 2 * MXG_REVNET_MAX_STAGES ? off.data() : nullptr, &S),
                           "mxg_revnet_layout_host");
            off.resize(combs.size() + aps.size());
        }
        size_t P() const { return combs.size(); }
        size_t A() const { return aps.size(); }
        size_t F() const { return combs.size() + aps.size(); }
    };
    void put(maxigpu::DeviceArray<double> &d, size_t stages, const std::vector<double> &h) {
        if (h.size() != V * stages) throw std::runtime_error("maxiReverbNetBank: a parameter array holds [voices][stages] values");
        maxigpu::check(mxg_sync(), "mxg_sync");  // a call still running reads the old values
        if (!h.empty()) d.upload(h.data(), h.size());
    }
    void fill(maxigpu::DeviceArray<double> &d, size_t stages, double value) { put(d, stages, std::vector<double>(V * stages, value)); }
    size_t V;
    Layout lay_;
    maxigpu::DeviceArray<double> rings_;
    maxigpu::DeviceArray<int32_t> idx_;
    maxigpu::DeviceArray<double> lp_, cfb_, cut_, afb_;
};

// ---- maxiDynamics (H:2625-2897) / maxiRMS (H:2579-2616) banks (K12): block-rate parameters per voice ------------------------
// (per-sample parameters: call mxg_dynamics_render with ps_flags).  Rings slot-major, [capacity][V]; the defaults are the
// reference's (500 ms and 1 s of samples at the sample rate in force at construction).  Times in ms as in the reference; the four
// attack / release times are one value per bank.
class maxiDynamicsBank {
public:
    enum ANALYSERS { PEAK = MXG_DYN_PEAK, RMS = MXG_DYN_RMS };
    explicit maxiDynamicsBank(size_t voices, size_t capRms = 0, size_t capLookahead = 0)
        : V(voices), capR(capRms ? capRms : msToSamps(500)), capL(capLookahead ? capLookahead : mxg_sample_rate()), rring_(voices * capR),
          lring_(voices * capL), rpos_(voices), lpos_(voices), running_(voices), dstH_(5 * voices), dstL_(5 * voices), istH_(7 * voices),
          istL_(7 * voices), ovf_(voices), win_(voices), look_(voices), an_(voices), tabH_(18), tabL_(18), window(voices, 0),
          lookahead(voices, 0), analyser(voices, RMS) {
        for (int e = 0; e < 2; e++) {  // fresh envelopes: previousValue = 1, firstTrigger = 1 for the three detectors (H:593-594)
            std::vector<double> d(5 * V, 0.0);
            std::vector<int64_t> i(7 * V, 0);
            std::fill(d.begin() + 2 * V, d.end(), 1.0);
            std::fill(i.begin() + 4 * V, i.end(), 1);
            (e ? dstL_ : dstH_).upload(d);
            (e ? istL_ : istH_).upload(i);
        }
        const double levels[4] = {0, 1, 1, 0}, times[3] = {10, -46692.0, 10}, curves[3] = {1, 1, 1};  // setupASR(10, 10)
        stagesHigh.assign(18, 0.0);
        maxigpu::check(mxg_envgen_stages_host(4, levels, times, curves, stagesHigh.data()), "mxg_envgen_stages_host");
        stagesLow = stagesHigh;
        const size_t w = msToSamps(50);  // rms.setup(500, 50)
        if (w <= capR) std::fill(window.begin(), window.end(), (uint32_t)w);
    }
    static size_t msToSamps(double ms) { return static_cast<size_t>(ms / 1000.0 * mxg_sample_rate()); }  // H:944-947
    void setAttackHigh(double ms) { setTime(stagesHigh, 0, ms); }
    void setReleaseHigh(double ms) { setTime(stagesHigh, 2, ms); }
    void setAttackLow(double ms) { setTime(stagesLow, 0, ms); }
    void setReleaseLow(double ms) { setTime(stagesLow, 2, ms); }
    void setLookAhead(double ms) {  // H:2844-2847, every voice
        const size_t n = msToSamps(ms);
        std::fill(lookahead.begin(), lookahead.end(), (uint32_t)(n < capL ? n : capL));
        dirty_ = true;
    }
    void setRMSWindowSize(double ms) {  // H:2859-2861, every voice: a request above the ring is ignored, the running sum is zeroed
        const size_t n = msToSamps(500.0 < ms ? 500.0 : ms);
        if (n <= capR) std::fill(window.begin(), window.end(), (uint32_t)n);
        running_.upload(std::vector<double>(V, 0.0));
        dirty_ = true;
    }
    void setInputAnalyser(ANALYSERS mode) {
        std::fill(analyser.begin(), analyser.end(), (int32_t)mode);
        dirty_ = true;
    }
    void setParams(const std::vector<double> &thresholdHigh, const std::vector<double> &ratioHigh, const std::vector<double> &kneeHigh,
                   const std::vector<double> &thresholdLow, const std::vector<double> &ratioLow, const std::vector<double> &kneeLow) {
        p_[0].upload(thresholdHigh); p_[1].upload(ratioHigh); p_[2].upload(kneeHigh);
        p_[3].upload(thresholdLow); p_[4].upload(ratioLow); p_[5].upload(kneeLow);
    }
    // compress(): the high section only, the signal is its own side chain
    void setCompress(const std::vector<double> &threshold, const std::vector<double> &ratio, const std::vector<double> &knee) {
        const std::vector<double> z(V, 0.0);
        setParams(threshold, ratio, knee, z, z, z);
    }
    // play(): d_control may be d_sig.  d_level_db (optional, [N][V]): the detector level in dB.
    void play(size_t N, const double *d_sig, const double *d_control, double *d_out, double *d_level_db = nullptr, void *stream = nullptr) {
        if (dirty_) {
            win_.upload(window); look_.upload(lookahead); an_.upload(analyser); tabH_.upload(stagesHigh); tabL_.upload(stagesLow);
            dirty_ = false;
        }
        maxigpu::check(mxg_dynamics_render(V, N, d_sig, d_control, p_[0].get(), p_[1].get(), p_[2].get(), p_[3].get(), p_[4].get(),
                                           p_[5].get(), 0, win_.get(), look_.get(), an_.get(), tabH_.get(), tabL_.get(), 3, rring_.get(),
                                           capR, lring_.get(), capL, rpos_.get(), lpos_.get(), running_.get(), dstH_.get(), istH_.get(),
                                           dstL_.get(), istL_.get(), ovf_.get(), d_out, d_level_db, stream), "mxg_dynamics_render");
    }
    void compress(size_t N, const double *d_sig, double *d_out, void *stream = nullptr) { play(N, d_sig, d_sig, d_out, nullptr, stream); }
    uint32_t *overflow() { return ovf_.get(); }  // device [V]
    size_t capacityRms() const { return capR; }
    size_t capacityLookahead() const { return capL; }

private:
    void setTime(std::vector<double> &tab, size_t index, double ms) {
        maxigpu::check(mxg_envgen_set_time_host(tab.data(), 3, index, ms), "mxg_envgen_set_time_host");
        dirty_ = true;
    }
    size_t V, capR, capL;
    maxigpu::DeviceArray<double> rring_, lring_;
    maxigpu::DeviceArray<int32_t> rpos_, lpos_;
    maxigpu::DeviceArray<double> running_, dstH_, dstL_;
    maxigpu::DeviceArray<int64_t> istH_, istL_;
    maxigpu::DeviceArray<uint32_t> ovf_, win_, look_;
    maxigpu::DeviceArray<int32_t> an_;
    maxigpu::DeviceArray<double> tabH_, tabL_, p_[6];
    bool dirty_ = true;

public:
    // host copies, in samples / per voice: edit and call touch() for per-voice settings
    std::vector<uint32_t> window, lookahead;
    std::vector<int32_t> analyser;
    std::vector<double> stagesHigh, stagesLow;  // [3][6]
    void touch() { dirty_ = true; }
};

class maxiRMSBank {
public:
    maxiRMSBank(size_t voices, size_t capacity)
        : V(voices), cap(capacity), ring_(voices * capacity), pos_(voices), running_(voices), ovf_(voices), win_(voices) {}
    void setWindowSize(double ms) {  // H:2590-2596, every voice
        const size_t n = maxiDynamicsBank::msToSamps(ms);
        if (n <= cap) win_.upload(std::vector<uint32_t>(V, (uint32_t)n));
        running_.upload(std::vector<double>(V, 0.0));
    }
    void play(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_rms_render(V, N, d_in, win_.get(), ring_.get(), cap, pos_.get(), running_.get(), ovf_.get(), d_out, stream),
                       "mxg_rms_render");
    }
    uint32_t *overflow() { return ovf_.get(); }

private:
    size_t V, cap;
    maxigpu::DeviceArray<double> ring_;
    maxigpu::DeviceArray<int32_t> pos_;
    maxigpu::DeviceArray<double> running_;
    maxigpu::DeviceArray<uint32_t> ovf_, win_;
};

// ---- analysis (H:969-1040, 1214-1250; kernel K16): what makes a trigger, a level or a held value FROM the audio --------
// V x (maxiZeroCrossingDetector, maxiZeroCrossingRate, maxiEnvelopeFollower, maxiSampleAndHold) over one input block [N][V]
// (mxg_analysis_render).  An output whose pointer is null is not rendered and its stage's state is untouched.  `capacity` is the
// size of the ring of crossings in samples (the reference sizes it from the sample rate at construction); the window defaults to
// it, the follower to setAttack(100), setRelease(100) at the sample rate in force at construction.  The ring holds one bit per
// slot: u64 [ceil(capacity / 64)][V].
class maxiAnalysisBank {
public:
    maxiAnalysisBank(size_t voices, size_t capacity = maxiSettings::sampleRate) : V(voices), cap(capacity) {
        if (cap < 1) throw std::runtime_error("maxiAnalysisBank: the ring needs at least one slot");
        window.assign(V, (uint32_t)cap);
        win_.upload(window);
        const double c = mxg_envfollow_coeff_host(100.0, (double)maxiSettings::sampleRate);
        attack_.upload(std::vector<double>(V, c));
        release_.upload(std::vector<double>(V, c));
        hold_.resize(V);
        reset();
    }
    void reset() {  // fresh objects: everything zero (the window, the coefficients and the hold times stay)
        prev_.resize(V); ring_.resize(((cap + 63) / 64) * V); pos_.resize(V); count_.resize(V); ovf_.resize(V);
        env_.resize(V); phase_.resize(V); value_.resize(V);
    }
    void setWindow(const std::vector<uint32_t> &samples) {  // per voice; 0 is refused, above the capacity: held there and counted
        if (samples.size() != V) throw std::runtime_error("maxiAnalysisBank::setWindow: one window per voice");
        maxigpu::check(mxg_analysis_window_host(V, samples.data(), cap), "mxg_analysis_window_host");
        window = samples;
        win_.upload(window);
    }
    void setWindow(uint32_t samples) { setWindow(std::vector<uint32_t>(V, samples)); }
    void setAttack(double ms) { attack_.upload(std::vector<double>(V, mxg_envfollow_coeff_host(ms, (double)maxiSettings::sampleRate))); }
    void setRelease(double ms) { release_.upload(std::vector<double>(V, mxg_envfollow_coeff_host(ms, (double)maxiSettings::sampleRate))); }
    void setHold(const std::vector<double> &ms) {
        if (ms.size() != V) throw std::runtime_error("maxiAnalysisBank::setHold: one hold time per voice");
        hold_.upload(ms);
    }
    void setHold(double ms) { setHold(std::vector<double>(V, ms)); }
    // d_hold_ms: null = the bank's per-voice hold times, else a hold time per sample [N][V]
    void render(size_t N, const double *d_in, double *d_zx, double *d_zcr, double *d_env, double *d_sah, const double *d_hold_ms = nullptr,
                void *stream = nullptr) {
        const int want = (d_zx ? MXG_ANA_WANT_ZX : 0) | (d_zcr ? MXG_ANA_WANT_ZCR : 0) | (d_env ? MXG_ANA_WANT_ENV : 0) |
                         (d_sah ? MXG_ANA_WANT_SAH : 0);
        maxigpu::check(mxg_analysis_render(V, N, d_in, want, prev_.get(), win_.get(), ring_.get(), cap, pos_.get(), count_.get(), ovf_.get(),
                                           attack_.get(), release_.get(), env_.get(), d_hold_ms ? d_hold_ms : hold_.get(), d_hold_ms ? 1 : 0,
                                           phase_.get(), value_.get(), d_zx, d_zcr, d_env, d_sah, stream), "mxg_analysis_render");
    }
    size_t voices() const { return V; }
    size_t capacity() const { return cap; }
    // state arrays on the device (include/maxigpu.h)
    double *previousX() { return prev_.get(); }
    uint64_t *ring() { return ring_.get(); }
    int32_t *ringPosition() { return pos_.get(); }
    int64_t *runningCount() { return count_.get(); }
    uint32_t *overflow() { return ovf_.get(); }
    double *envelope() { return env_.get(); }
    double *holdPhase() { return phase_.get(); }
    double *holdValue() { return value_.get(); }
    std::vector<uint32_t> window;  // host copy, in samples

private:
    size_t V, cap;
    maxigpu::DeviceArray<double> prev_, env_, phase_, value_, attack_, release_, hold_;
    maxigpu::DeviceArray<uint64_t> ring_;
    maxigpu::DeviceArray<int32_t> pos_;
    maxigpu::DeviceArray<int64_t> count_;
    maxigpu::DeviceArray<uint32_t> ovf_, win_;
};

// ---- phase-coupled oscillator sets (H:1628-1808; kernel K17) ---------------------------------------------------------
// S x maxiKuramotoOscillatorSet -- asynchronous: maxiAsyncKuramotoOscillator -- of N = 1 .. 64 oscillators each
// (mxg_kuramoto_render).  play() is the reference's play(freq, K) for B samples: the mix block [B][S], and on request what
// getPhase(i) returns after each sample [B][S][N].  freq and K are one value per set, or device blocks [B][S] written by the
// other banks.  setPhase / setPhases act between two blocks, as the reference's do between two samples; on asynchronous sets
// they raise the set's flag, which the next play() consumes on its first sample.  meanfield: the tolerance mode that forms the
// coupling sum from the set's summed sines and cosines (N pairs per sample instead of N * N sines).
class maxiKuramotoBank {
public:
    maxiKuramotoBank(size_t sets, size_t N, bool meanfield = false, bool asynchronous = false)
        : S(sets), N_(N), mode((meanfield ? MXG_KURA_MEANFIELD : 0) | (asynchronous ? MXG_KURA_ASYNC : 0)) {
        if (N_ < 1 || N_ > 64) throw std::runtime_error("maxiKuramotoBank: a set has 1 .. 64 oscillators");
        freq_.resize(S);
        K_.resize(S);
        reset();
    }
    void reset() {  // fresh sets: phases 0, gathered phases 0, flags down
        phase_.resize(S * N_);
        if (mode & MXG_KURA_ASYNC) { gathered_.resize(S * N_); update_.resize(S); }
    }
    size_t sets() const { return S; }
    size_t size() const { return N_; }
    void setFreq(const std::vector<double> &f) { per_set(f, freq_, "setFreq"); }
    void setFreq(double f) { setFreq(std::vector<double>(S, f)); }
    void setK(const std::vector<double> &k) { per_set(k, K_, "setK"); }
    void setK(double k) { setK(std::vector<double>(S, k)); }
    // [S][N], set-major
    void setPhases(const std::vector<double> &phases) {
        if (phases.size() != S * N_) throw std::runtime_error("maxiKuramotoBank::setPhases: S * N phases");
        maxigpu::check(mxg_sync(), "mxg_sync");
        phase_.upload(phases);
        if (mode & MXG_KURA_ASYNC) update_.upload(std::vector<int32_t>(S, 1));
    }
    void setPhase(double phase, size_t oscillatorIdx, size_t set) {
        if (set >= S || oscillatorIdx >= N_) throw std::runtime_error("maxiKuramotoBank::setPhase: no such oscillator");
        maxigpu::check(mxg_sync(), "mxg_sync");
        phase_.upload(&phase, 1, set * N_ + oscillatorIdx);
        const int32_t one = 1;
        if (mode & MXG_KURA_ASYNC) update_.upload(&one, 1, set);
    }
    std::vector<double> phases() const {  // getPhase(i) of every set, [S][N]
        maxigpu::check(mxg_sync(), "mxg_sync");
        return phase_.download();
    }
    // d_mix [B][S] and / or d_phases_out [B][S][N] (null: not rendered); d_freq / d_K: null = the bank's per-set values, else a
    // block [B][S]
    void play(size_t B, double *d_mix, double *d_phases_out = nullptr, const double *d_freq = nullptr, const double *d_K = nullptr,
              void *stream = nullptr) {
        const int want = (d_mix ? MXG_KURA_WANT_MIX : 0) | (d_phases_out ? MXG_KURA_WANT_PHASES : 0);
        maxigpu::check(mxg_kuramoto_render(mode, S, N_, B, d_freq ? d_freq : freq_.get(), d_freq ? 1 : 0, d_K ? d_K : K_.get(), d_K ? 1 : 0,
                                           phase_.get(), gathered_.get(), update_.get(), want, d_mix, d_phases_out, stream),
                       "mxg_kuramoto_render");
    }
    // state arrays on the device (include/maxigpu.h)
    double *phase() { return phase_.get(); }
    double *gathered() { return gathered_.get(); }
    int32_t *update() { return update_.get(); }

private:
    void per_set(const std::vector<double> &v, maxigpu::DeviceArray<double> &d, const char *what) {
        if (v.size() != S) throw std::runtime_error(std::string("maxiKuramotoBank::") + what + ": one value per set");
        maxigpu::check(mxg_sync(), "mxg_sync");
        d.upload(v);
    }
    size_t S, N_;
    int mode;
    maxigpu::DeviceArray<double> freq_, K_, phase_, gathered_;
    maxigpu::DeviceArray<int32_t> update_;
};

// maxiKuramotoBank for sets of N = 1 .. 1024 oscillators (mxg_kuramoto_wide_render, kernel K26: one workgroup per set, one lane
// per oscillator).  The same surface; it pays from N = 65 on -- up to 64 both give the same bits and maxiKuramotoBank packs
// several sets into a wavefront.  The exact form is N * N sines per set and sample; meanfield is N sine / cosine pairs.
class maxiKuramotoWideBank {
public:
    maxiKuramotoWideBank(size_t sets, size_t N, bool meanfield = false, bool asynchronous = false)
        : S(sets), N_(N), mode((meanfield ? MXG_KURA_MEANFIELD : 0) | (asynchronous ? MXG_KURA_ASYNC : 0)) {
        if (N_ < 1 || N_ > MXG_KURA_WIDE_MAX_N) throw std::runtime_error("maxiKuramotoWideBank: a set has 1 .. 1024 oscillators");
        freq_.resize(S);
        K_.resize(S);
        reset();
    }
    void reset() {  // fresh sets: phases 0, gathered phases 0, flags down
        phase_.resize(S * N_);
        if (mode & MXG_KURA_ASYNC) { gathered_.resize(S * N_); update_.resize(S); }
    }
    size_t sets() const { return S; }
    size_t size() const { return N_; }
    void setFreq(const std::vector<double> &f) { per_set(f, freq_, "setFreq"); }
    void setFreq(double f) { setFreq(std::vector<double>(S, f)); }
    void setK(const std::vector<double> &k) { per_set(k, K_, "setK"); }
    void setK(double k) { setK(std::vector<double>(S, k)); }
    // [S][N], set-major
    void setPhases(const std::vector<double> &phases) {
        if (phases.size() != S * N_) throw std::runtime_error("maxiKuramotoWideBank::setPhases: S * N phases");
        maxigpu::check(mxg_sync(), "mxg_sync");
        phase_.upload(phases);
        if (mode & MXG_KURA_ASYNC) update_.upload(std::vector<int32_t>(S, 1));
    }
    void setPhase(double phase, size_t oscillatorIdx, size_t set) {
        if (set >= S || oscillatorIdx >= N_) throw std::runtime_error("maxiKuramotoWideBank::setPhase: no such oscillator");
        maxigpu::check(mxg_sync(), "mxg_sync");
        phase_.upload(&phase, 1, set * N_ + oscillatorIdx);
        const int32_t one = 1;
        if (mode & MXG_KURA_ASYNC) update_.upload(&one, 1, set);
    }
    std::vector<double> phases() const {  // getPhase(i) of every set, [S][N]
        maxigpu::check(mxg_sync(), "mxg_sync");
        return phase_.download();
    }
    // d_mix [B][S] and / or d_phases_out [B][S][N] (null: not rendered); d_freq / d_K: null = the bank's per-set values, else a
    // block [B][S]
    void play(size_t B, double *d_mix, double *d_phases_out = nullptr, const double *d_freq = nullptr, const double *d_K = nullptr,
              void *stream = nullptr) {
        const int want = (d_mix ? MXG_KURA_WANT_MIX : 0) | (d_phases_out ? MXG_KURA_WANT_PHASES : 0);
        maxigpu::check(mxg_kuramoto_wide_render(mode, S, N_, B, d_freq ? d_freq : freq_.get(), d_freq ? 1 : 0, d_K ? d_K : K_.get(),
                                                d_K ? 1 : 0, phase_.get(), gathered_.get(), update_.get(), want, d_mix, d_phases_out,
                                                stream),
                       "mxg_kuramoto_wide_render");
    }
    // state arrays on the device (include/maxigpu.h)
    double *phase() { return phase_.get(); }
    double *gathered() { return gathered_.get(); }
    int32_t *update() { return update_.get(); }

private:
    void per_set(const std::vector<double> &v, maxigpu::DeviceArray<double> &d, const char *what) {
        if (v.size() != S) throw std::runtime_error(std::string("maxiKuramotoWideBank::") + what + ": one value per set");
        maxigpu::check(mxg_sync(), "mxg_sync");
        d.upload(v);
    }
    size_t S, N_;
    int mode;
    maxigpu::DeviceArray<double> freq_, K_, phase_, gathered_;
    maxigpu::DeviceArray<int32_t> update_;
};

// ---- shapers, cross-fade, select and line (H:1046-1139, 1491-1617, 2018-2088; kernel K18) ----------------------------
// The small classes that sit BETWEEN the other banks: every block is [N][V] on the device, so a chain such as oscillator ->
// distortion -> filter, or "cross-fade two banks by a line", never leaves it.  The first three are stateless.
// V x maxiNonlinearity / maxiDistortion (mxg_shape_render): one method per reference call.  The scalar / vector overloads take
// per-voice parameters; the pointer overloads a device block [N][V] (a parameter per sample).  d_out may be d_in.
class maxiShaperBank {
public:
    explicit maxiShaperBank(size_t voices) : V(voices) {}
    size_t voices() const { return V; }
    void hardclip(size_t N, const double *d_in, double *d_out, void *stream = nullptr) { run(MXG_SHAPE_HARDCLIP, N, d_in, nullptr, nullptr, 0, d_out, stream); }
    void softclip(size_t N, const double *d_in, double *d_out, void *stream = nullptr) { run(MXG_SHAPE_SOFTCLIP, N, d_in, nullptr, nullptr, 0, d_out, stream); }
    void fastatan(size_t N, const double *d_in, double *d_out, void *stream = nullptr) { run(MXG_SHAPE_FASTATAN, N, d_in, nullptr, nullptr, 0, d_out, stream); }
    void fastAtanDist(size_t N, const double *d_in, const std::vector<double> &shape, double *d_out, void *stream = nullptr) {
        per_voice(shape, a_, "fastAtanDist");
        run(MXG_SHAPE_FASTATANDIST, N, d_in, a_.get(), nullptr, 0, d_out, stream);
    }
    void fastAtanDist(size_t N, const double *d_in, double shape, double *d_out, void *stream = nullptr) {
        fastAtanDist(N, d_in, std::vector<double>(V, shape), d_out, stream);
    }
    void fastAtanDist(size_t N, const double *d_in, const double *d_shape, double *d_out, void *stream = nullptr) {
        run(MXG_SHAPE_FASTATANDIST, N, d_in, d_shape, nullptr, 1, d_out, stream);
    }
    void atanDist(size_t N, const double *d_in, const std::vector<double> &shape, double *d_out, void *stream = nullptr) {
        per_voice(shape, a_, "atanDist");
        std::vector<double> norm(V);
        for (size_t v = 0; v < V; v++) norm[v] = mxg_atan_norm_host(shape[v]);  // 1.0 / atan(shape), host libm
        b_.upload(norm);
        run(MXG_SHAPE_ATANDIST, N, d_in, a_.get(), b_.get(), 0, d_out, stream);
    }
    void atanDist(size_t N, const double *d_in, double shape, double *d_out, void *stream = nullptr) {
        atanDist(N, d_in, std::vector<double>(V, shape), d_out, stream);
    }
    void atanDist(size_t N, const double *d_in, const double *d_shape, double *d_out, void *stream = nullptr) {
        run(MXG_SHAPE_ATANDIST, N, d_in, d_shape, nullptr, 1, d_out, stream);
    }
    void asymclip(size_t N, const double *d_in, const std::vector<double> &a, const std::vector<double> &b, double *d_out, void *stream = nullptr) {
        per_voice(a, a_, "asymclip");
        per_voice(b, b_, "asymclip");
        run(MXG_SHAPE_ASYMCLIP, N, d_in, a_.get(), b_.get(), 0, d_out, stream);
    }
    void asymclip(size_t N, const double *d_in, double a, double b, double *d_out, void *stream = nullptr) {
        asymclip(N, d_in, std::vector<double>(V, a), std::vector<double>(V, b), d_out, stream);
    }
    void asymclip(size_t N, const double *d_in, const double *d_a, const double *d_b, double *d_out, void *stream = nullptr) {
        run(MXG_SHAPE_ASYMCLIP, N, d_in, d_a, d_b, 1, d_out, stream);
    }

private:
    void per_voice(const std::vector<double> &p, maxigpu::DeviceArray<double> &d, const char *what) {
        if (p.size() != V) throw std::runtime_error(std::string("maxiShaperBank::") + what + ": one value per voice");
        maxigpu::check(mxg_sync(), "mxg_sync");  // (an earlier render may still read the last values)
        d.upload(p);
    }
    void run(int mode, size_t N, const double *d_in, const double *a, const double *b, int ps, double *d_out, void *stream) {
        maxigpu::check(mxg_shape_render(mode, V, N, d_in, a, b, ps, d_out, stream), "mxg_shape_render");
    }
    size_t V;
    maxigpu::DeviceArray<double> a_, b_;
};

// V x maxiXFade::xfade over C channels (mxg_xfade_render): d_ch1, d_ch2, d_out are [C][N][V]; the xfader is one value per
// voice, or a device block [N][V].  d_out may be d_ch1 or d_ch2.
class maxiXFadeBank {
public:
    explicit maxiXFadeBank(size_t voices, size_t channels = 1) : V(voices), C(channels) {
        if (C < 1 || C > MXG_XFADE_MAX_C) throw std::runtime_error("maxiXFadeBank: 1 .. 8 channels");
    }
    size_t voices() const { return V; }
    size_t channels() const { return C; }
    void xfade(size_t N, const double *d_ch1, const double *d_ch2, const std::vector<double> &xfader, double *d_out, void *stream = nullptr) {
        if (xfader.size() != V) throw std::runtime_error("maxiXFadeBank::xfade: one xfader per voice");
        maxigpu::check(mxg_sync(), "mxg_sync");
        xf_.upload(xfader);
        maxigpu::check(mxg_xfade_render(C, V, N, d_ch1, d_ch2, xf_.get(), 0, d_out, stream), "mxg_xfade_render");
    }
    void xfade(size_t N, const double *d_ch1, const double *d_ch2, double xfader, double *d_out, void *stream = nullptr) {
        xfade(N, d_ch1, d_ch2, std::vector<double>(V, xfader), d_out, stream);
    }
    void xfade(size_t N, const double *d_ch1, const double *d_ch2, const double *d_xfader, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_xfade_render(C, V, N, d_ch1, d_ch2, d_xfader, 1, d_out, stream), "mxg_xfade_render");
    }

private:
    size_t V, C;
    maxigpu::DeviceArray<double> xf_;
};

// V x maxiSelect (interpolate = false) / maxiSelectX (true) over K = 1 .. 64 values (mxg_select_render).  setValues: K
// constants for every voice, or K and [K][V]; playSignals reads K device blocks [K][N][V] instead.  A NaN index (undefined in the
// reference) reads element 0 and is counted per voice in nanCount().
class maxiSelectBank {
public:
    explicit maxiSelectBank(size_t voices, bool interpolate = false) : V(voices), X(interpolate), K(0) { nan_.resize(V); }
    size_t voices() const { return V; }
    void setValues(const std::vector<double> &values) {  // K constants shared by the voices
        std::vector<double> kv(values.size() * V);
        for (size_t k = 0; k < values.size(); k++)
            for (size_t v = 0; v < V; v++) kv[k * V + v] = values[k];
        setValues(values.size(), kv);
    }
    void setValues(size_t values, const std::vector<double> &kv) {  // [K][V]
        if (values < 1 || values > MXG_SELECT_MAX_K || kv.size() != values * V) throw std::runtime_error("maxiSelectBank::setValues: 1 .. 64 values, [K][V]");
        maxigpu::check(mxg_sync(), "mxg_sync");
        K = values;
        values_.upload(kv);
    }
    void play(size_t N, const double *d_index, bool normalised, double *d_out, void *stream = nullptr) {
        if (!K) throw std::runtime_error("maxiSelectBank::play: setValues first");
        maxigpu::check(mxg_select_render(X ? 1 : 0, K, V, N, d_index, values_.get(), 0, normalised ? 1 : 0, nan_.get(), d_out, stream), "mxg_select_render");
    }
    void playSignals(size_t N, const double *d_index, size_t values, const double *d_values, bool normalised, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_select_render(X ? 1 : 0, values, V, N, d_index, d_values, 1, normalised ? 1 : 0, nan_.get(), d_out, stream), "mxg_select_render");
    }
    std::vector<uint32_t> nanCount() const {
        maxigpu::check(mxg_sync(), "mxg_sync");
        return nan_.download();
    }

private:
    size_t V;
    bool X;
    size_t K;
    maxigpu::DeviceArray<double> values_;
    maxigpu::DeviceArray<uint32_t> nan_;
};

// V x maxiLine (mxg_line_render).  prepare / triggerEnable act between two blocks, as the reference's do between two samples;
// prepare keeps the reference's quirk (lineValue takes the PREVIOUS lineStart).  play(N, d_trig, ...) reads a trigger block
// [N][V]; play(N, trigger, ...) is the line.play(1) idiom.
class maxiLineBank {
public:
    explicit maxiLineBank(size_t voices) : V(voices) { reset(); }
    size_t voices() const { return V; }
    void reset() {  // fresh objects: lineValue 0, lastTrigVal -1, inc 0, one-shot, triggers disabled
        par_.assign(5 * V, 0.0);
        st_.assign(4 * V, 0.0);
        for (size_t v = 0; v < V; v++) { par_[3 * V + v] = 1.0; st_[V + v] = -1.0; }
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_par_.upload(par_);
        d_st_.upload(st_);
    }
    void prepare(const std::vector<double> &start, const std::vector<double> &end, const std::vector<double> &durationMs,
                 const std::vector<int32_t> &isOneShot, const std::vector<int32_t> *mask = nullptr) {
        if (start.size() != V || end.size() != V || durationMs.size() != V || isOneShot.size() != V || (mask && mask->size() != V))
            throw std::runtime_error("maxiLineBank::prepare: one value per voice");
        pull();
        maxigpu::check(mxg_line_prepare_host(V, start.data(), end.data(), durationMs.data(), isOneShot.data(), mask ? mask->data() : nullptr,
                                             (double)maxiSettings::sampleRate, par_.data(), st_.data()), "mxg_line_prepare_host");
        d_par_.upload(par_);
        d_st_.upload(st_);
    }
    void prepare(double start, double end, double durationMs, bool isOneShot) {
        prepare(std::vector<double>(V, start), std::vector<double>(V, end), std::vector<double>(V, durationMs), std::vector<int32_t>(V, isOneShot ? 1 : 0));
    }
    void triggerEnable(const std::vector<double> &on) {
        if (on.size() != V) throw std::runtime_error("maxiLineBank::triggerEnable: one value per voice");
        pull();
        for (size_t v = 0; v < V; v++) par_[4 * V + v] = on[v] > 0.0 ? 1.0 : 0.0;
        d_par_.upload(par_);
    }
    void triggerEnable(double on) { triggerEnable(std::vector<double>(V, on)); }
    std::vector<bool> isLineComplete() {
        pull();
        std::vector<bool> done(V);
        for (size_t v = 0; v < V; v++) done[v] = st_[3 * V + v] != 0.0;
        return done;
    }
    void play(size_t N, const double *d_trig, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_line_render(V, N, d_trig, 0.0, d_par_.get(), d_st_.get(), d_out, stream), "mxg_line_render");
    }
    void play(size_t N, double trigger, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_line_render(V, N, nullptr, trigger, d_par_.get(), d_st_.get(), d_out, stream), "mxg_line_render");
    }
    // parameter and state arrays on the device (include/maxigpu.h): [5][V] and [4][V]
    double *parameters() { return d_par_.get(); }
    double *state() { return d_st_.get(); }

private:
    void pull() {  // the state as the last render left it
        maxigpu::check(mxg_sync(), "mxg_sync");
        st_ = d_st_.download();
    }
    size_t V;
    std::vector<double> par_, st_;
    maxigpu::DeviceArray<double> d_par_, d_st_;
};

// ---- the classic core classes: maxiDyn, maxiEnvelope, maxiLagExp<double>, maxiMap / maxiConvert (kernel K23) --------------
// V x maxiDyn (mxg_dyn_gate_render / mxg_dyn_compress_render).  gate() and compressor() take one value per voice; compress() runs
// the same step on the members the four setters left (setAttack / setRelease in ms store pow(0.01, ...), which compress() uses as
// 1 + attack: the reference's quirk).  Gate and compressor share one state, as the members of one maxiDyn are.  d_out is distinct
// from d_in.  The *_blocks overloads read a device block [N][V] for every parameter whose MXG_CLASSIC_PS_* bit is set.
class maxiDynBank {
public:
    explicit maxiDynBank(size_t voices) : V(voices), ratio_(voices, 0.0), threshold_(voices, 0.0), attack_(voices, 0.0), release_(voices, 0.0) {
        d_dst_.resize(3 * V);
        d_ist_.resize(4 * V);
    }
    size_t voices() const { return V; }
    void gate(size_t N, const double *d_in, const std::vector<double> &threshold, const std::vector<int64_t> &holdtime,
              const std::vector<double> &attack, const std::vector<double> &release, double *d_out, void *stream = nullptr) {
        per_voice(threshold, thr_, "gate");
        per_voice(attack, att_, "gate");
        per_voice(release, rel_, "gate");
        if (holdtime.size() != V) throw std::runtime_error("maxiDynBank::gate: one value per voice");
        hold_.upload(holdtime);
        gate_blocks(N, d_in, thr_.get(), att_.get(), rel_.get(), 0, hold_.get(), d_out, stream);
    }
    void gate(size_t N, const double *d_in, double threshold, long holdtime, double attack, double release, double *d_out, void *stream = nullptr) {
        gate(N, d_in, std::vector<double>(V, threshold), std::vector<int64_t>(V, holdtime), std::vector<double>(V, attack),
             std::vector<double>(V, release), d_out, stream);
    }
    void gate_blocks(size_t N, const double *d_in, const double *d_threshold, const double *d_attack, const double *d_release, int ps_flags,
                     const int64_t *d_holdtime, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_dyn_gate_render(V, N, d_in, d_threshold, d_attack, d_release, ps_flags, d_holdtime, d_dst_.get(), d_ist_.get(), d_out,
                                           stream), "mxg_dyn_gate_render");
    }
    void compressor(size_t N, const double *d_in, const std::vector<double> &ratio, const std::vector<double> &threshold,
                    const std::vector<double> &attack, const std::vector<double> &release, double *d_out, void *stream = nullptr) {
        per_voice(ratio, rat_, "compressor");
        per_voice(threshold, thr_, "compressor");
        per_voice(attack, att_, "compressor");
        per_voice(release, rel_, "compressor");
        std::vector<double> mk(V);
        for (size_t v = 0; v < V; v++) mk[v] = mxg_dyn_makeup_host(ratio[v]);  // 1 + log(ratio), host libm
        mk_.upload(mk);
        compressor_blocks(N, d_in, rat_.get(), mk_.get(), thr_.get(), att_.get(), rel_.get(), 0, d_out, stream);
    }
    void compressor(size_t N, const double *d_in, double ratio, double threshold, double attack, double release, double *d_out, void *stream = nullptr) {
        compressor(N, d_in, std::vector<double>(V, ratio), std::vector<double>(V, threshold), std::vector<double>(V, attack),
                   std::vector<double>(V, release), d_out, stream);
    }
    // d_makeup: mxg_dyn_makeup_host of every ratio, in the layout of d_ratio
    void compressor_blocks(size_t N, const double *d_in, const double *d_ratio, const double *d_makeup, const double *d_threshold,
                           const double *d_attack, const double *d_release, int ps_flags, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_dyn_compress_render(V, N, d_in, d_ratio, d_makeup, d_threshold, d_attack, d_release, ps_flags, d_dst_.get(),
                                               d_ist_.get(), d_out, stream), "mxg_dyn_compress_render");
    }
    void compress(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        compressor(N, d_in, ratio_, threshold_, attack_, release_, d_out, stream);
    }
    void setAttack(double attackMS) { attack_.assign(V, mxg_dyn_coeff_host(attackMS, (double)maxiSettings::sampleRate)); }
    void setRelease(double releaseMS) { release_.assign(V, mxg_dyn_coeff_host(releaseMS, (double)maxiSettings::sampleRate)); }
    void setThreshold(double thresholdI) { threshold_.assign(V, thresholdI); }
    void setRatio(double ratioF) { ratio_.assign(V, ratioF); }
    // state arrays on the device (include/maxigpu.h): double [3][V] and int64 [4][V]
    double *state() { return d_dst_.get(); }
    int64_t *phases() { return d_ist_.get(); }

private:
    void per_voice(const std::vector<double> &p, maxigpu::DeviceArray<double> &d, const char *what) {
        if (p.size() != V) throw std::runtime_error(std::string("maxiDynBank::") + what + ": one value per voice");
        maxigpu::check(mxg_sync(), "mxg_sync");  // (an earlier render may still read the last values)
        d.upload(p);
    }
    size_t V;
    std::vector<double> ratio_, threshold_, attack_, release_;
    maxigpu::DeviceArray<double> thr_, att_, rel_, rat_, mk_, d_dst_;
    maxigpu::DeviceArray<int64_t> hold_, d_ist_;
};

// V x maxiEnvelope (mxg_envelope_line_render).  segments: one table (value, time, value, time ...) for every voice, or [S][V] with
// a count per voice.  trigger() acts between two blocks; line(N, d_trig, ...) reads a trigger block [N][V] whose non-zero values
// perform trigger(index, amp) before that sample.  A trigger index outside [0, count - 2] is refused.
class maxiEnvelopeBank {
public:
    maxiEnvelopeBank(size_t voices, const std::vector<double> &segments) : V(voices), S(segments.size()) {
        std::vector<double> sv(S * V);
        for (size_t s = 0; s < S; s++)
            for (size_t v = 0; v < V; v++) sv[s * V + v] = segments[s];
        init(sv, std::vector<int32_t>(V, (int32_t)S));
    }
    maxiEnvelopeBank(size_t voices, size_t entries, const std::vector<double> &segments_sv, const std::vector<int32_t> &count) : V(voices), S(entries) {
        init(segments_sv, count);
    }
    size_t voices() const { return V; }
    void trigger(const std::vector<int32_t> &index, const std::vector<double> &amp, const std::vector<int32_t> *mask = nullptr) {
        if (index.size() != V || amp.size() != V || (mask && mask->size() != V)) throw std::runtime_error("maxiEnvelopeBank::trigger: one value per voice");
        maxigpu::check(mxg_sync(), "mxg_sync");
        std::vector<double> dst = d_dst_.download();
        std::vector<int32_t> ist = d_ist_.download();
        maxigpu::check(mxg_envelope_trigger_host(V, index.data(), amp.data(), mask ? mask->data() : nullptr, count_.data(), dst.data(), ist.data()),
                       "mxg_envelope_trigger_host");
        d_dst_.upload(dst);
        d_ist_.upload(ist);
    }
    void trigger(int index, double amp) { trigger(std::vector<int32_t>(V, index), std::vector<double>(V, amp)); }
    void line(size_t N, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_envelope_line_render(V, N, S, d_seg_.get(), d_count_.get(), nullptr, nullptr, nullptr, d_dst_.get(), d_ist_.get(), d_out,
                                                stream), "mxg_envelope_line_render");
    }
    void line(size_t N, const double *d_trig, int trig_index, double trig_amp, double *d_out, void *stream = nullptr) {
        for (size_t v = 0; v < V; v++)
            if (trig_index < 0 || trig_index > count_[v] - 2) throw std::runtime_error("maxiEnvelopeBank::line: trigger index outside [0, count - 2]");
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_tix_.upload(std::vector<int32_t>(V, trig_index));
        d_tamp_.upload(std::vector<double>(V, trig_amp));
        maxigpu::check(mxg_envelope_line_render(V, N, S, d_seg_.get(), d_count_.get(), d_trig, d_tix_.get(), d_tamp_.get(), d_dst_.get(), d_ist_.get(),
                                                d_out, stream), "mxg_envelope_line_render");
    }
    // state arrays on the device (include/maxigpu.h): double [2][V] = amplitude, startval; int32 [2][V] = valindex, isPlaying
    double *state() { return d_dst_.get(); }
    int32_t *indices() { return d_ist_.get(); }

private:
    void init(const std::vector<double> &sv, const std::vector<int32_t> &count) {
        if (S < 2 || S > MXG_ENVELOPE_MAX_S || sv.size() != S * V || count.size() != V) throw std::runtime_error("maxiEnvelopeBank: 2 .. 64 entries, [S][V], one count per voice");
        for (int32_t c : count)
            if (c < 2 || (size_t)c > S) throw std::runtime_error("maxiEnvelopeBank: a count outside 2 .. S");
        count_ = count;
        d_seg_.upload(sv);
        d_count_.upload(count);
        d_dst_.resize(2 * V);
        d_ist_.resize(2 * V);
    }
    size_t V, S;
    std::vector<int32_t> count_;
    maxigpu::DeviceArray<double> d_seg_, d_dst_, d_tamp_;
    maxigpu::DeviceArray<int32_t> d_count_, d_ist_, d_tix_;
};

// V x maxiLagExp<double> (mxg_lag_render): val = (alpha * x) + (alphaReciprocal * val) over a block; alpha and alphaReciprocal are
// independent, as in the reference (init sets both, setAlpha only alpha).  d_out is distinct from d_in.
class maxiLagExpBank {
public:
    maxiLagExpBank(size_t voices, double alpha = 0.5, double val = 0.0) : V(voices) { init(alpha, val); }
    size_t voices() const { return V; }
    void init(double alpha, double val) {
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_alpha_.upload(std::vector<double>(V, alpha));
        d_recip_.upload(std::vector<double>(V, 1.0 - alpha));
        d_val_.upload(std::vector<double>(V, val));
    }
    void setAlpha(double alpha) { maxigpu::check(mxg_sync(), "mxg_sync"); d_alpha_.upload(std::vector<double>(V, alpha)); }
    void setAlphaReciprocal(double r) { maxigpu::check(mxg_sync(), "mxg_sync"); d_recip_.upload(std::vector<double>(V, r)); }
    void setVal(double val) { maxigpu::check(mxg_sync(), "mxg_sync"); d_val_.upload(std::vector<double>(V, val)); }
    void addSample(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_lag_render(V, N, d_in, d_alpha_.get(), d_recip_.get(), 0, d_val_.get(), d_out, stream), "mxg_lag_render");
    }
    void addSample(size_t N, const double *d_in, const double *d_alpha, const double *d_alpha_reciprocal, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_lag_render(V, N, d_in, d_alpha, d_alpha_reciprocal, 1, d_val_.get(), d_out, stream), "mxg_lag_render");
    }
    std::vector<double> value() const {
        maxigpu::check(mxg_sync(), "mxg_sync");
        return d_val_.download();
    }

private:
    size_t V;
    maxigpu::DeviceArray<double> d_alpha_, d_recip_, d_val_;
};

// R writable maxiSample slots on the device (mxg_sample_pool_alloc, K25): loopRecord (H:706-721) over blocks [N][R] that other
// banks rendered, one play head per slot -- play() or playLoop() -- fused behind the record head in the reference's call order,
// and normalise (C:1126-1137).  Bit-exact and independent of how the samples are split into calls; a record index outside
// [0, len) reads 0, stores nothing and is counted (dropped()).  deviceSamples(r) / getLength(r) feed mxg_sample_render*.
class maxiLooperBank {
public:
    maxiLooperBank(size_t slots, size_t capacity) : R(slots), cap_(capacity), len_(slots, capacity) {
        maxigpu::check(mxg_init(-1), "mxg_init");
        pool_ = mxg_sample_pool_alloc(R, cap_, &stride_);
        if (!pool_) throw std::runtime_error(std::string("mxg_sample_pool_alloc: ") + mxg_last_error());
        d_len_.resize(R);
        pushLengths();
        d_recpos_.resize(R);
        d_lag_.resize(R);
        d_dropped_.resize(R);
        d_position_.upload(std::vector<double>(R, (double)capacity - 1.0));
        d_mix_.upload(std::vector<double>(R, 0.5));
        d_start_.upload(std::vector<double>(R, 0.0));
        d_end_.upload(std::vector<double>(R, 1.0));
        d_pstart_.upload(std::vector<double>(R, 0.0));
        d_pend_.upload(std::vector<double>(R, 1.0));
    }
    maxiLooperBank(const maxiLooperBank &) = delete;
    maxiLooperBank &operator=(const maxiLooperBank &) = delete;
    ~maxiLooperBank() { mxg_sample_pool_free(pool_); }
    size_t slots() const { return R; }
    size_t capacity() const { return cap_; }
    size_t stride() const { return stride_; }
    double *deviceSamples(size_t r) const { return pool_ + r * stride_; }
    const uint64_t *deviceLengths() const { return d_len_.get(); }  // uint64 [R] on the device (mxg_granular_pool_render's d_len)
    size_t getLength(size_t r) const { return (size_t)len_[r]; }
    // maxiSample::setSample (H:670-678) on one slot: the data, zeros up to the capacity, position = len - 1
    void setSample(size_t r, const std::vector<double> &data) {
        if (data.empty() || data.size() > cap_) throw std::invalid_argument("maxiLooperBank::setSample: the data does not fit the slot");
        std::vector<double> full(cap_, 0.0);
        std::copy(data.begin(), data.end(), full.begin());
        maxigpu::check(mxg_sync(), "mxg_sync");
        maxigpu::check(mxg_memcpy_h2d(deviceSamples(r), full.data(), cap_ * sizeof(double), nullptr), "mxg_memcpy_h2d");
        len_[r] = data.size();
        pushLengths();
        const double pos = (double)data.size() - 1.0;
        d_position_.upload(&pos, 1, r);
    }
    void setLength(size_t r, size_t n) {
        const uint64_t old = len_[r];
        len_[r] = n;
        try {
            pushLengths();
        } catch (...) {
            len_[r] = old;
            throw;
        }
    }
    void trigger() {  // C:597-600 on every slot
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_position_.upload(std::vector<double>(R, 0.0));
        d_recpos_.upload(std::vector<double>(R, 0.0));
    }
    void setRecordMix(double mix) { spread(d_mix_, mix); }
    void setLoop(double start, double end) { spread(d_start_, start); spread(d_end_, end); }
    void setPlayLoop(double start, double end) { spread(d_pstart_, start); spread(d_pend_, end); }
    // d_enable: [N][R] doubles (perSample) or [R]; non-zero = true
    void loopRecord(size_t N, const double *d_in, const double *d_enable, bool perSample, void *stream = nullptr) {
        render(N, d_in, d_enable, perSample, MXG_LOOPER_PLAY_NONE, nullptr, stream);
    }
    void play(size_t N, const double *d_in, const double *d_enable, bool perSample, double *d_out, void *stream = nullptr) {
        render(N, d_in, d_enable, perSample, MXG_SMP_PLAY, d_out, stream);
    }
    void playLoop(size_t N, const double *d_in, const double *d_enable, bool perSample, double *d_out, void *stream = nullptr) {
        render(N, d_in, d_enable, perSample, MXG_SMP_PLAYLOOP, d_out, stream);
    }
    void normalise(double maxLevel = 0.99, void *stream = nullptr) {
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_level_.upload(std::vector<double>(R, maxLevel));
        maxigpu::check(mxg_sample_pool_normalise(R, pool_, stride_, cap_, d_len_.get(), d_level_.get(), stream), "mxg_sample_pool_normalise");
    }
    std::vector<double> download(size_t r) const {
        std::vector<double> h(getLength(r));
        maxigpu::check(mxg_sync(), "mxg_sync");
        maxigpu::check(mxg_memcpy_d2h(h.data(), deviceSamples(r), h.size() * sizeof(double), nullptr), "mxg_memcpy_d2h");
        return h;
    }
    std::vector<uint32_t> dropped() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_dropped_.download(); }
    std::vector<double> recordPosition() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_recpos_.download(); }
    std::vector<double> position() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_position_.download(); }
    std::vector<double> lagValue() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_lag_.download(); }

private:
    void pushLengths() { maxigpu::check(mxg_sample_pool_lengths(R, cap_, len_.data(), d_len_.get()), "mxg_sample_pool_lengths"); }
    void spread(maxigpu::DeviceArray<double> &a, double x) {
        maxigpu::check(mxg_sync(), "mxg_sync");
        a.upload(std::vector<double>(R, x));
    }
    void render(size_t N, const double *d_in, const double *d_enable, bool perSample, int mode, double *d_out, void *stream) {
        maxigpu::check(mxg_looprec_render(R, N, pool_, stride_, cap_, d_len_.get(), d_in, d_enable, perSample ? 1 : 0, d_mix_.get(),
                                          d_start_.get(), d_end_.get(), d_recpos_.get(), d_lag_.get(), mode, d_pstart_.get(), d_pend_.get(),
                                          d_position_.get(), d_out, d_dropped_.get(), stream),
                       "mxg_looprec_render");
    }
    size_t R, cap_, stride_ = 0;
    double *pool_ = nullptr;
    std::vector<uint64_t> len_;
    maxigpu::DeviceArray<uint64_t> d_len_;
    maxigpu::DeviceArray<uint32_t> d_dropped_;
    maxigpu::DeviceArray<double> d_recpos_, d_lag_, d_position_, d_mix_, d_start_, d_end_, d_pstart_, d_pend_, d_level_;
};

// S granular streams that each read their OWN slot of a maxiLooperBank's pool (K27, mxg_granular_pool_render): the reference's
// maxiTimeStretch / maxiPitchShift / maxiStretch objects after setSample(), maxiStretch with its loop points (L/maxiGrains.h:445,
// :493-509) and playAtPosition (:531-539).  A parameter is [S] on the device, or a block [N][S] another bank wrote (perSample = true):
// a block is read at every sample.  Every render writes the [N][S] block maxiMixBank::stereo takes.  Bit-exact, and independent of
// how the samples are split into calls.  A render only enqueues while stream s reads slot s; with any other assignment the C-ABI reads
// the slot indices back before it launches, so the call waits for the stream.  The bank must not outlive its pool.
class maxiGrainPoolBank {
public:
    maxiGrainPoolBank(size_t streams, const maxiLooperBank &pool, int window_kind = 0)
        : S(streams), pool_(pool), kind_(window_kind), slot_(streams), loop_(2 * streams), whole_(streams, 1) {
        maxigpu::check(mxg_init(-1), "mxg_init");
        d_st_.resize(4 * S);
        d_gst_.resize(32 * S);
        d_slot_.resize(S);
        d_loop_.resize(2 * S);
        for (size_t s = 0; s < S; s++) {
            slot_[s] = (uint32_t)(s % pool_.slots());
            loop_[s] = 0;
            loop_[S + s] = pool_.getLength(slot_[s]);
        }
    }
    maxiGrainPoolBank(const maxiGrainPoolBank &) = delete;
    maxiGrainPoolBank &operator=(const maxiGrainPoolBank &) = delete;
    ~maxiGrainPoolBank() {
        for (auto &p : plans_) mxg_grain_plan_destroy(p.second);
    }
    size_t streams() const { return S; }
    size_t getLength(size_t s) const { return pool_.getLength(slot_[at(s)]); }
    uint32_t getSlot(size_t s) const { return slot_[at(s)]; }
    // setSample() of stream s: slot r from now on, no live grains; stretch = maxiStretch::setSample (:466-478): position, looper and
    // the loop are reset too
    void setSlot(size_t s, size_t r, bool stretch = true) {
        if (s >= S || r >= pool_.slots()) throw std::invalid_argument("maxiGrainPoolBank::setSlot: the stream or the slot does not exist");
        maxigpu::check(mxg_sync(), "mxg_sync");
        slot_[s] = (uint32_t)r;
        std::vector<double> g = d_gst_.download();
        for (size_t i = 0; i < 32; i++) g[i * S + s] = 0.0;
        d_gst_.upload(g);
        if (stretch) {
            std::vector<double> st = d_st_.download();
            st[s] = st[S + s] = 0.0;
            d_st_.upload(st);
            loop_[s] = 0;
            loop_[S + s] = pool_.getLength(r);
            whole_[s] = 1;
        }
        dirty_ = true;
    }
    // setLoopStart + setLoopEnd (:493-501): NaN, a negative value, loopStart >= loopEnd and loopEnd > len are refused
    void setLoop(size_t s, double start01, double end01) {
        uint64_t ls = 0, le = 0;
        maxigpu::check(mxg_stretch_loop_host(getLength(s), start01, end01, &ls, &le), "mxg_stretch_loop_host");
        loop_[s] = ls;
        loop_[S + s] = le;
        whole_[s] = 0;
        dirty_ = true;
    }
    void setLoopStart(size_t s, double val) {
        uint64_t ls = 0, le = 0;
        maxigpu::check(mxg_stretch_loop_host(getLength(s), val, 1.0, &ls, &le), "mxg_stretch_loop_host");
        followLengths();
        if (ls >= loop_[S + s]) throw std::invalid_argument("maxiGrainPoolBank::setLoopStart: loopStart >= loopEnd");
        loop_[s] = ls;
        whole_[s] = 0;
        dirty_ = true;
    }
    void setLoopEnd(size_t s, double val) {
        uint64_t ls = 0, le = 0;
        maxigpu::check(mxg_stretch_loop_host(getLength(s), 0.0, val, &ls, &le), "mxg_stretch_loop_host");
        if (le <= loop_[s]) throw std::invalid_argument("maxiGrainPoolBank::setLoopEnd: loopStart >= loopEnd");
        loop_[S + s] = le;
        whole_[s] = 0;
        dirty_ = true;
    }
    unsigned long getLoopStart(size_t s) const { return (unsigned long)loop_[at(s)]; }
    unsigned long getLoopEnd(size_t s) {
        followLengths();
        return (unsigned long)loop_[S + at(s)];
    }
    void setPosition(size_t s, double pos) {  // :488-491
        at(s);
        const double n = (double)getLength(s);
        double p = pos * n;
        p = p < 0.0 ? 0.0 : (p > n - 1.0 ? n - 1.0 : p);
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_st_.upload(&p, 1, s);
    }
    std::vector<double> getPosition() const {
        maxigpu::check(mxg_sync(), "mxg_sync");
        std::vector<double> st = d_st_.download();
        st.resize(S);
        return st;
    }
    std::vector<double> getNormalisedPosition() const {
        std::vector<double> p = getPosition();
        for (size_t s = 0; s < S; s++) p[s] /= (double)getLength(s);
        return p;
    }
    std::vector<double> state() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_st_.download(); }    // [4][S]
    std::vector<double> grains() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_gst_.download(); }  // [4][8][S]
    // maxiTimeStretch::play (:341-355); d_rnd int32 [S][Rn] or null
    void timestretch(size_t N, const double *d_speed, bool perSample, double grainLength, int overlaps, const double *d_posMod, bool posModPerSample,
                     const int32_t *d_rnd, size_t Rn, double *d_out, void *stream = nullptr) {
        render(0, N, d_speed, perSample, nullptr, false, grainLength, overlaps, d_posMod, posModPerSample, d_rnd, Rn, d_out, stream);
    }
    // maxiPitchShift::play (:412-430)
    void pitchshift(size_t N, const double *d_speed, bool perSample, double grainLength, int overlaps, const double *d_posMod, bool posModPerSample,
                    double *d_out, void *stream = nullptr) {
        render(3, N, d_speed, perSample, nullptr, false, grainLength, overlaps, d_posMod, posModPerSample, nullptr, 0, d_out, stream);
    }
    // maxiStretch::play (:512-530) inside each stream's loop points
    void stretch(size_t N, const double *d_pitch, bool pitchPerSample, const double *d_rate, bool ratePerSample, double grainLength, int overlaps,
                 const double *d_posMod, bool posModPerSample, const int32_t *d_rnd, size_t Rn, double *d_out, void *stream = nullptr) {
        render(1, N, d_pitch, pitchPerSample, d_rate, ratePerSample, grainLength, overlaps, d_posMod, posModPerSample, d_rnd, Rn, d_out, stream);
    }
    // maxiTimeStretch::playAtPosition (:359-367): d_pos [N][S]
    void playAtPosition(size_t N, const double *d_pos, double grainLength, int overlaps, double *d_out, void *stream = nullptr) {
        render(2, N, d_pos, false, nullptr, false, grainLength, overlaps, nullptr, false, nullptr, 0, d_out, stream);
    }
    // maxiStretch::playAtPosition (:531-539): d_pos [S], or [N][S] with posPerSample
    void stretchAtPosition(size_t N, const double *d_pitch, bool pitchPerSample, const double *d_pos, bool posPerSample, double grainLength,
                           int overlaps, double *d_out, void *stream = nullptr) {
        render(4, N, d_pitch, pitchPerSample, d_pos, posPerSample, grainLength, overlaps, nullptr, false, nullptr, 0, d_out, stream);
    }

private:
    size_t at(size_t s) const {
        if (s >= S) throw std::out_of_range("maxiGrainPoolBank: the stream does not exist");
        return s;
    }
    // a stream on its whole slot has loopEnd = the slot's length NOW (the pool's setSample / setLength may have changed it), as the
    // reference's setSample re-derives it; a loop that was set stays as set
    void followLengths() {
        for (size_t s = 0; s < S; s++)
            if (whole_[s] && loop_[S + s] != pool_.getLength(slot_[s])) {
                loop_[S + s] = pool_.getLength(slot_[s]);
                dirty_ = true;
            }
    }
    mxg_grain_plan *plan(double grainLength) {
        for (auto &p : plans_)
            if (p.first == grainLength) return p.second;
        mxg_grain_plan *pl = mxg_grain_plan_create(kind_, grainLength, 44100);  // maxiSample::setSample: mySampleRate = 44100 (H:676)
        if (!pl) throw std::runtime_error(std::string("mxg_grain_plan_create: ") + mxg_last_error());
        plans_.push_back(std::make_pair(grainLength, pl));
        return pl;
    }
    void render(int mode, size_t N, const double *d_a, bool psA, const double *d_b, bool psB, double grainLength, int overlaps, const double *d_pm,
                bool psP, const int32_t *d_rnd, size_t Rn, double *d_out, void *stream) {
        followLengths();
        if (dirty_) {
            maxigpu::check(mxg_sync(), "mxg_sync");
            d_slot_.upload(slot_);
            d_loop_.upload(loop_);
            dirty_ = false;
        }
        // the indices were checked in setSlot.  Stream s on slot s needs no d_slot, and then the call only enqueues; any other assignment
        // hands the C-ABI the device array, which it reads back before it launches (that call waits for the stream)
        bool identity = S <= pool_.slots();
        for (size_t s = 0; identity && s < S; s++) identity = slot_[s] == s;
        const int ps = (psA && mode != 2 ? MXG_GPOOL_PS_A : 0) | (psB ? MXG_GPOOL_PS_B : 0) | (psP && d_pm ? MXG_GPOOL_PS_POSMOD : 0);
        maxigpu::check(mxg_granular_pool_render(plan(grainLength), mode, S, N, pool_.deviceSamples(0), pool_.stride(), pool_.capacity(), pool_.slots(),
                                                pool_.deviceLengths(), identity ? nullptr : d_slot_.get(), mode == 1 ? d_loop_.get() : nullptr, overlaps, d_a, d_b, d_pm, ps,
                                                d_rnd, Rn, d_st_.get(), d_gst_.get(), d_out, stream),
                       "mxg_granular_pool_render");
    }
    size_t S;
    const maxiLooperBank &pool_;
    int kind_;
    bool dirty_ = true;
    std::vector<uint32_t> slot_;
    std::vector<uint64_t> loop_;
    std::vector<char> whole_;  // the stream's loop is its whole slot
    std::vector<std::pair<double, mxg_grain_plan *>> plans_;
    maxigpu::DeviceArray<uint32_t> d_slot_;
    maxigpu::DeviceArray<uint64_t> d_loop_;
    maxigpu::DeviceArray<double> d_st_, d_gst_;
};

// V x maxiMap / maxiConvert (mxg_map_render): stateless, flat over the block; d_out may be d_in.  Ranges are one value for the
// bank or one per voice.  linlin and clamp are the reference's bits; the other four use the device's pow / log / log10.
class maxiMapBank {
public:
    explicit maxiMapBank(size_t voices) : V(voices) {}
    size_t voices() const { return V; }
    void linlin(size_t N, const double *d_in, double inMin, double inMax, double outMin, double outMax, double *d_out, void *stream = nullptr) {
        ranged(MXG_MAP_LINLIN, N, d_in, spread(inMin, inMax, outMin, outMax), d_out, stream);
    }
    void linexp(size_t N, const double *d_in, double inMin, double inMax, double outMin, double outMax, double *d_out, void *stream = nullptr) {
        ranged(MXG_MAP_LINEXP, N, d_in, spread(inMin, inMax, outMin, outMax), d_out, stream);
    }
    void explin(size_t N, const double *d_in, double inMin, double inMax, double outMin, double outMax, double *d_out, void *stream = nullptr) {
        ranged(MXG_MAP_EXPLIN, N, d_in, spread(inMin, inMax, outMin, outMax), d_out, stream);
    }
    void clamp(size_t N, const double *d_in, double low, double high, double *d_out, void *stream = nullptr) {
        ranged(MXG_MAP_CLAMP, N, d_in, spread(low, high, 0.0, 0.0), d_out, stream);
    }
    // range4v: [4][V] = inMin, inMax, outMin, outMax per voice
    void ranged(int mode, size_t N, const double *d_in, const std::vector<double> &range4v, double *d_out, void *stream = nullptr) {
        if (range4v.size() != 4 * V) throw std::runtime_error("maxiMapBank: a range is [4][V]");
        std::vector<double> aux(V);
        maxigpu::check(mxg_map_range_host(mode, V, range4v.data(), aux.data()), "mxg_map_range_host");
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_range_.upload(range4v);
        d_aux_.upload(aux);
        maxigpu::check(mxg_map_render(mode, V, N, d_in, d_range_.get(), d_aux_.get(), d_out, stream), "mxg_map_render");
    }
    void ampToDbs(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_map_render(MXG_MAP_AMPTODBS, V, N, d_in, nullptr, nullptr, d_out, stream), "mxg_map_render");
    }
    void dbsToAmp(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_map_render(MXG_MAP_DBSTOAMP, V, N, d_in, nullptr, nullptr, d_out, stream), "mxg_map_render");
    }

private:
    std::vector<double> spread(double a, double b, double c, double d) const {
        std::vector<double> r(4 * V);
        for (size_t v = 0; v < V; v++) { r[v] = a; r[V + v] = b; r[2 * V + v] = c; r[3 * V + v] = d; }
        return r;
    }
    size_t V;
    maxigpu::DeviceArray<double> d_range_, d_aux_;
};

// V x maxiPolyBLEP (mxg_polyblep_render, K20): one waveform for the bank, a pulse width and a phase per voice, the phase carried
// from call to call.  set_waveform / set_pulse_width / sync act between two blocks, as the reference's setters do between two
// samples.  render(N, d_freq, per_sample, ...) reads one frequency per voice [V] or a block [N][V].
class maxiPolyBLEPBank {
public:
    explicit maxiPolyBLEPBank(size_t voices, double sampleRate = (double)maxiSettings::sampleRate) : V(voices), sr_(sampleRate) {
        d_t_.upload(std::vector<double>(V, 0.0));  // the reference's constructor: SINE, pulse width 0.5, t = 0
    }
    size_t voices() const { return V; }
    void set_waveform(int waveform) {
        if (waveform < 0 || waveform >= MXG_PBLEP_WAVEFORMS) throw std::runtime_error("maxiPolyBLEPBank::set_waveform: one of MXG_PBLEP_*");
        wf_ = waveform;
    }
    int waveform() const { return wf_; }
    void set_sample_rate(double sampleRate) { sr_ = sampleRate; }
    void set_pulse_width(const std::vector<double> &pw) {
        if (pw.size() != V) throw std::runtime_error("maxiPolyBLEPBank::set_pulse_width: one value per voice");
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_pw_.upload(pw);
        has_pw_ = true;
    }
    void set_pulse_width(double pw) { set_pulse_width(std::vector<double>(V, pw)); }
    // PolyBLEP::sync: t = phase - (int64)phase, a negative phase t = phase + (1 - (int64)phase)
    static double wrap(double phase) { return phase >= 0 ? phase - std::trunc(phase) : phase + (1 - std::trunc(phase)); }
    void sync(const std::vector<double> &phases) {
        if (phases.size() != V) throw std::runtime_error("maxiPolyBLEPBank::sync: one value per voice");
        std::vector<double> t(V);
        for (size_t v = 0; v < V; v++) t[v] = wrap(phases[v]);
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_t_.upload(t);
    }
    void sync(double phase) { sync(std::vector<double>(V, phase)); }
    void render(size_t N, const double *d_freq, bool per_sample, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_polyblep_render(wf_, V, N, d_freq, per_sample ? 1 : 0, has_pw_ ? d_pw_.get() : nullptr, sr_, d_t_.get(), d_out, stream),
                       "mxg_polyblep_render");
    }
    // the phases on the device [V]
    double *phases() { return d_t_.get(); }

private:
    size_t V;
    double sr_;
    int wf_ = MXG_PBLEP_SINE;
    bool has_pw_ = false;
    maxigpu::DeviceArray<double> d_t_, d_pw_;
};

// V x maxiKick / maxiSnare / maxiHats (src/libs/maxiSynths.h; mxg_drum_render, K21): KIND is MXG_DRUM_KICK / SNARE / HATS.  The
// setters take the reference's units (ms through mxg_env_coeff_host, cutoff / resonance through the coefficient hosts); the four
// switches are one value for the bank.  State, carried from call to call, all zero in a fresh bank: phase [V], dst [2][V], ist
// int64 [6][V] (mxg_env_render's layout), fst [3][V].  cutoff / resonance start at 0.0 where the reference leaves them
// uninitialised (lores clamps them to 10 Hz and 1).  The hats' SVF takes setFilterCutoff / setFilterResonance (the reference's
// filter.setCutoff / setResonance; the constructor: 8000, 1); their cutoff / resonance are, as in the reference, never read.
template <int KIND>
class maxiDrumBank {
public:
    bool inverse = false, useDistortion = false, useFilter = (KIND == MXG_DRUM_SNARE), useLimiter = false;

    explicit maxiDrumBank(size_t voices)
        : V(voices), pitch_(V, KIND == MXG_DRUM_KICK ? 200. : (KIND == MXG_DRUM_SNARE ? 800. : 12000.)), env_(4 * V), hold_(V, 1),
          shape_(V, 0.), cutoff_(V, 0.), res_(V, 0.), gain_(V, 1.), svf_cutoff_(V, 8000.), svf_res_(V, 1.), d_phase_(V), d_dst_(2 * V),
          d_ist_(6 * V), d_fst_(3 * V) {
        setAttack(0);
        setDecay(KIND == MXG_DRUM_KICK ? 1 : 20);
        setSustain(KIND == MXG_DRUM_KICK ? 1 : (KIND == MXG_DRUM_SNARE ? 0.05 : 0.1));
        setRelease(KIND == MXG_DRUM_KICK ? 500 : 300);
    }
    size_t voices() const { return V; }
    void setAttack(double ms) { row(0, mxg_env_coeff_host(0, ms)); }  // (0: divides by zero inside pow, attack = 1)
    void setDecay(double ms) { row(1, mxg_env_coeff_host(1, ms)); }
    void setSustain(double level) { row(2, level); }
    void setRelease(double ms) { row(3, mxg_env_coeff_host(2, ms)); }
    void setHoldtime(long samples) { fill(hold_, (int64_t)samples); }
    void setPitch(double v) { fill(pitch_, v); }
    void setPitch(const std::vector<double> &v) { assign(pitch_, v); }
    void setDistortion(double v) { fill(shape_, v); }
    void setCutoff(double v) { fill(cutoff_, v); }
    void setResonance(double v) { fill(res_, v); }
    void setGain(double v) { fill(gain_, v); }
    void setFilterCutoff(double v) { fill(svf_cutoff_, v); }
    void setFilterResonance(double v) { fill(svf_res_, v); }
    int flags() const {
        return (inverse ? MXG_DRUM_INVERSE : 0) | (useDistortion ? MXG_DRUM_DISTORTION : 0) | (useFilter ? MXG_DRUM_FILTER : 0) |
               (useLimiter ? MXG_DRUM_LIMITER : 0);
    }
    // N x play() per voice.  d_trig: doubles [N][V] (per_voice) or [N], non-zero = trigger() before that play(), null = never (a
    // maxiClockBank's tick block fits); d_rand: int32 [N][V], the rand() draws of snare and hats (null for the kick).
    void render(size_t N, const double *d_trig, bool per_voice, const int32_t *d_rand, double *d_out, void *stream = nullptr) {
        if (dirty_) {
            std::vector<double> coef((KIND == MXG_DRUM_HATS ? 5 : 3) * V);
            if (KIND == MXG_DRUM_HATS) maxigpu::check(mxg_svf_coeffs_host(V, svf_cutoff_.data(), svf_res_.data(), coef.data()), "mxg_svf_coeffs_host");
            else maxigpu::check(mxg_filter_coeffs_host(MXG_FLT_LORES, V, cutoff_.data(), res_.data(), coef.data()), "mxg_filter_coeffs_host");
            maxigpu::check(mxg_sync(), "mxg_sync");
            d_pitch_.upload(pitch_); d_env_.upload(env_); d_hold_.upload(hold_); d_shape_.upload(shape_); d_coef_.upload(coef); d_gain_.upload(gain_);
            dirty_ = false;
        }
        maxigpu::check(mxg_drum_render(KIND, flags(), V, N, d_trig, per_voice ? 1 : 0, d_rand, d_pitch_.get(), d_env_.get(), d_hold_.get(),
                                       d_shape_.get(), d_coef_.get(), d_gain_.get(), d_phase_.get(), d_dst_.get(), d_ist_.get(), d_fst_.get(),
                                       d_out, stream), "mxg_drum_render");
    }
    // the state on the device (get / set with DeviceArray::download / upload, i.e. mxg_memcpy_*)
    maxigpu::DeviceArray<double> &phase() { return d_phase_; }
    maxigpu::DeviceArray<double> &dstate() { return d_dst_; }
    maxigpu::DeviceArray<int64_t> &istate() { return d_ist_; }
    maxigpu::DeviceArray<double> &fstate() { return d_fst_; }

private:
    template <typename T>
    void fill(std::vector<T> &a, T v) { std::fill(a.begin(), a.end(), v); dirty_ = true; }
    void assign(std::vector<double> &a, const std::vector<double> &v) {
        if (v.size() != V) throw std::runtime_error("maxiDrumBank: one value per voice");
        a = v;
        dirty_ = true;
    }
    void row(int r, double v) { std::fill(env_.begin() + r * V, env_.begin() + (r + 1) * V, v); dirty_ = true; }
    size_t V;
    bool dirty_ = true;
    std::vector<double> pitch_, env_;
    std::vector<int64_t> hold_;
    std::vector<double> shape_, cutoff_, res_, gain_, svf_cutoff_, svf_res_;
    maxigpu::DeviceArray<double> d_phase_, d_dst_;
    maxigpu::DeviceArray<int64_t> d_ist_;
    maxigpu::DeviceArray<double> d_fst_, d_pitch_, d_env_, d_shape_, d_coef_, d_gain_;
    maxigpu::DeviceArray<int64_t> d_hold_;
};
using maxiKickBank = maxiDrumBank<MXG_DRUM_KICK>;
using maxiSnareBank = maxiDrumBank<MXG_DRUM_SNARE>;
using maxiHatsBank = maxiDrumBank<MXG_DRUM_HATS>;

// V x maxiClock (src/libs/maxiClock.h; mxg_clock_render): render(N, d_tick) is N x ticker() per voice and writes the tick block
// [N][V] of 1.0 / 0.0, which a drum bank's render takes as d_trig.  lastCount is only read, as in the reference.
class maxiClockBank {
public:
    explicit maxiClockBank(size_t voices)
        : V(voices), bpm_(V, 120.), ticks_(V, 1), d_clk_(V), d_playhead_(V), d_last_(V), d_count_(V) { setTempo(120.); }
    size_t voices() const { return V; }
    void setTempo(double bpm) { std::fill(bpm_.begin(), bpm_.end(), bpm); push(); }
    void setTicksPerBeat(int ticksPerBeat) { std::fill(ticks_.begin(), ticks_.end(), ticksPerBeat); push(); }
    void setLastCount(int n) { maxigpu::check(mxg_sync(), "mxg_sync"); d_last_.upload(std::vector<int32_t>(V, n)); }
    void render(size_t N, double *d_tick, void *stream = nullptr) {
        maxigpu::check(mxg_clock_render(V, N, d_bps_.get(), d_clk_.get(), d_last_.get(), d_playhead_.get(), d_count_.get(), d_tick, stream),
                       "mxg_clock_render");
    }
    std::vector<int64_t> playHead() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_playhead_.download(); }
    std::vector<int32_t> currentCount() const { maxigpu::check(mxg_sync(), "mxg_sync"); return d_count_.download(); }
    maxigpu::DeviceArray<double> &phase() { return d_clk_; }

private:
    void push() {
        std::vector<double> bps(V);
        for (size_t v = 0; v < V; v++) bps[v] = (bpm_[v] / 60.) * ticks_[v];  // setTempo: bps = (bpm/60.)*ticks
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_bps_.upload(bps);
    }
    size_t V;
    std::vector<double> bpm_;
    std::vector<int> ticks_;
    maxigpu::DeviceArray<double> d_clk_, d_bps_;
    maxigpu::DeviceArray<int64_t> d_playhead_;
    maxigpu::DeviceArray<int32_t> d_last_, d_count_;
};

// S x (maxiAccelerator + maxiAtomBook + maxiAtomBookPlayer) (src/libs/maxiAtoms.h; kernel K22, mxg_atoms_*): every stream owns a queue of
// at most `capacity` live atoms and, optionally, a book.  fillNextBuffer / play write the float32 block [S][N] on the device, each
// stream's buffer contiguous; accumulate: the sum starts from what d_out holds (the reference's +=).  onset MXG_ATOM_ONSET_BLOCK is the
// reference's, MXG_ATOM_ONSET_SAMPLE (an extension) starts a due atom on its own sample.
class maxiAtomBank {
public:
    struct BookAtom {  // what a maxiGaborAtom holds
        float position, length, amp, frequency, phase;
    };
    maxiAtomBank(size_t streams, size_t capacity, const std::vector<std::vector<BookAtom>> &books = {}, const std::vector<uint32_t> &numSamples = {},
                 const std::vector<float> &raw = {})
        : S(streams), Q(capacity) {
        std::vector<int64_t> start(S + 1, 0);
        if (!books.empty() && books.size() != S) throw std::runtime_error("maxiAtomBank: one book per stream");
        for (size_t s = 0; s < S && !books.empty(); s++) start[s + 1] = start[s] + (int64_t)books[s].size();
        const size_t A = (size_t)start[S];
        std::vector<float> rows(5 * A);
        for (size_t s = 0, k = 0; s < S && !books.empty(); s++)
            for (const BookAtom &a : books[s]) {
                rows[k] = a.position, rows[A + k] = a.length, rows[2 * A + k] = a.amp, rows[3 * A + k] = a.frequency, rows[4 * A + k] = a.phase;
                k++;
            }
        std::vector<uint32_t> ns(S, 1);
        for (size_t s = 0; s < S && s < numSamples.size(); s++) ns[s] = numSamples[s];
        h_ = mxg_atoms_bank_create(S, Q, start.data(), rows.data(), ns.data(), raw.data(), raw.size());
        if (!h_) throw std::runtime_error(std::string("mxg_atoms_bank_create: ") + mxg_last_error());
    }
    ~maxiAtomBank() { mxg_atoms_bank_destroy(h_); }
    maxiAtomBank(const maxiAtomBank &) = delete;
    maxiAtomBank &operator=(const maxiAtomBank &) = delete;
    size_t streams() const { return S; }
    uint32_t appendRaw(const std::vector<float> &floats) {
        uint32_t at = 0;
        maxigpu::check(mxg_atoms_raw_append(h_, floats.data(), floats.size(), &at), "mxg_atoms_raw_append");
        return at;
    }
    // addAtom(atom, offset) on one stream: a raw atom of `length` floats from the pool ...
    void addAtom(int32_t stream, uint32_t rawOffset, uint32_t length, uint32_t offset = 0) {
        const int32_t kind = MXG_ATOM_RAW;
        maxigpu::check(mxg_atoms_add(h_, 1, &stream, &kind, &length, &offset, nullptr, &rawOffset), "mxg_atoms_add");
    }
    // ... or createGabor's arguments, synthesised on the device
    void addGabor(int32_t stream, float freq, float sampleRate, uint32_t length, float startPhase, float amp, uint32_t offset = 0) {
        const int32_t kind = MXG_ATOM_GABOR;
        const float par[4] = {freq, sampleRate, startPhase, amp};
        maxigpu::check(mxg_atoms_add(h_, 1, &stream, &kind, &length, &offset, par, nullptr), "mxg_atoms_add");
    }
    void fillNextBuffer(size_t N, float *d_out, int onset = MXG_ATOM_ONSET_BLOCK, bool accumulate = true, void *stream = nullptr) {
        maxigpu::check(mxg_atoms_fill(h_, N, d_out, onset, accumulate ? 1 : 0, stream), "mxg_atoms_fill");
    }
    void play(size_t N, float *d_out, int onset = MXG_ATOM_ONSET_BLOCK, bool accumulate = true, void *stream = nullptr) {
        maxigpu::check(mxg_atoms_play(h_, N, d_out, onset, accumulate ? 1 : 0, stream), "mxg_atoms_play");
    }
    std::vector<int64_t> sampleIdx() const {
        std::vector<int64_t> v(S);
        maxigpu::check(mxg_atoms_state(h_, v.data(), nullptr, nullptr, nullptr, nullptr, nullptr), "mxg_atoms_state");
        return v;
    }
    std::vector<int32_t> liveCount() const {
        std::vector<int32_t> v(S);
        maxigpu::check(mxg_atoms_state(h_, nullptr, nullptr, v.data(), nullptr, nullptr, nullptr), "mxg_atoms_state");
        return v;
    }

private:
    size_t S, Q;
    mxg_atoms_bank *h_ = nullptr;
};

// ---- sequencers (H:564-596, 1953-2013, 2093-2262; kernel K15): what tells the other banks WHEN ----------------------
namespace maxigpu {
// lists of doubles as the table form of mxg_seq_render / mxg_seq_signal: doubles [P][L] + int32 lengths [P] on the device
class SeqTable {
public:
    void set(const std::vector<std::vector<double>> &rows, bool ratios) {
        if (rows.empty()) throw std::runtime_error("SeqTable: no list");
        P = rows.size();
        L = 0;
        for (const auto &r : rows) L = r.size() > L ? r.size() : L;
        std::vector<double> tab(P * L, 0.0);
        std::vector<int32_t> len(P);
        for (size_t p = 0; p < P; p++) {
            if (rows[p].empty()) throw std::runtime_error("SeqTable: an empty list");
            len[p] = (int32_t)rows[p].size();
            for (size_t i = 0; i < rows[p].size(); i++) tab[p * L + i] = rows[p][i];
        }
        if (ratios) {  // maxiRatioSeq::playTrig's boundaries, on the host
            std::vector<double> norm(P * L);
            check(mxg_seq_ratio_host(P, L, len.data(), tab.data(), norm.data()), "mxg_seq_ratio_host");
            tab.swap(norm);
        }
        tab_.resize(tab.size(), false);
        tab_.upload(tab);
        len_.resize(len.size(), false);
        len_.upload(len);
    }
    const double *tab() const { return tab_.get(); }
    const int32_t *len() const { return len_.get(); }
    size_t P = 0, L = 0;

private:
    DeviceArray<double> tab_;
    DeviceArray<int32_t> len_;
};
}  // namespace maxigpu

// V fused sequencers: clock -> maxiRatioSeq::playTrig -> playValues | maxiStep::pull -> maxiZXToPulse::play (mxg_seq_render).
// Patterns and value lists are block-constant; per voice: setPattern / setValueList / setStep / setHold.  The output blocks are
// what maxiEnvGenBank::play (per_voice) and mxg_osc_render (fps = 1) read.
class maxiSeqBank {
public:
    enum ValueMode { VALUES = MXG_SEQ_VAL_VALUES, STEP = MXG_SEQ_VAL_STEP };
    maxiSeqBank(size_t voices, const std::vector<std::vector<double>> &times, const std::vector<std::vector<double>> &values = {})
        : V(voices), clk_(voices), dst_(5 * voices), ist_(6 * voices) {
        std::vector<double> d(5 * V, 0.0);
        std::vector<int64_t> i(6 * V, 0);
        for (size_t v = 0; v < V; v++) { d[V + v] = d[3 * V + v] = 1.0; i[v] = i[3 * V + v] = i[4 * V + v] = i[5 * V + v] = 1; }
        dst_.upload(d); ist_.upload(i);
        setTimes(times);
        if (!values.empty()) setValues(values);
    }
    void setTimes(const std::vector<std::vector<double>> &times) { pat_.set(times, true); }
    void setValues(const std::vector<std::vector<double>> &values) { val_.set(values, false); }
    void setPattern(const std::vector<int32_t> &sel) { sel_.upload(sel); has_sel_ = true; }
    void setValueList(const std::vector<int32_t> &sel) { vsel_.upload(sel); has_vsel_ = true; }
    void setStep(const std::vector<double> &step) { step_.upload(step); has_step_ = true; }
    void setHold(const std::vector<double> &samples) { hold_.upload(samples); has_hold_ = true; }
    // internal clock maxiOsc::phasor(d_freq[v]); any of d_trig / d_val / d_gate may be null (that stage does not run)
    void render(size_t N, const double *d_freq, double *d_trig, double *d_val, double *d_gate, ValueMode mode = VALUES,
                void *stream = nullptr) {
        run(N, d_freq, clk_.get(), nullptr, 0, d_trig, d_val, d_gate, mode, stream);
    }
    // external clock: d_phase [N][V] (per_voice) or one shared [N]
    void renderPhase(size_t N, const double *d_phase, bool per_voice, double *d_trig, double *d_val, double *d_gate,
                     ValueMode mode = VALUES, void *stream = nullptr) {
        run(N, nullptr, nullptr, d_phase, per_voice ? 1 : 0, d_trig, d_val, d_gate, mode, stream);
    }
    double *clockPhase() { return clk_.get(); }
    double *stateDoubles() { return dst_.get(); }
    int64_t *stateInts() { return ist_.get(); }

private:
    void run(size_t N, const double *f, double *clk, const double *ph, int pv, double *t, double *x, double *g, ValueMode mode, void *stream) {
        maxigpu::check(mxg_seq_render(V, N, f, clk, ph, pv, pat_.tab(), pat_.len(), pat_.P, pat_.L, has_sel_ ? sel_.get() : nullptr, mode,
                                      val_.tab(), val_.len(), val_.P, val_.L, has_vsel_ ? vsel_.get() : nullptr,
                                      has_step_ ? step_.get() : nullptr, has_hold_ ? hold_.get() : nullptr, dst_.get(), ist_.get(), t, x, g,
                                      stream), "mxg_seq_render");
    }
    size_t V;
    maxigpu::SeqTable pat_, val_;
    maxigpu::DeviceArray<double> clk_, dst_, step_, hold_;
    maxigpu::DeviceArray<int64_t> ist_;
    maxigpu::DeviceArray<int32_t> sel_, vsel_;
    bool has_sel_ = false, has_vsel_ = false, has_step_ = false, has_hold_ = false;
};

namespace maxigpu {
// one of the reference's sequencing classes driven by device signals [N][V] (mxg_seq_signal)
class SeqSignalBank {
public:
    void setValues(const std::vector<std::vector<double>> &values) { val_.set(values, false); }
    void setValueList(const std::vector<int32_t> &sel) { vsel_.upload(sel); has_vsel_ = true; }

protected:
    SeqSignalBank(int kind, size_t voices) : kind_(kind), V(voices), dst_(3 * voices), ist_(2 * voices) {
        std::vector<double> d(3 * V, 0.0);
        std::vector<int64_t> i(2 * V, 0);
        for (size_t v = 0; v < V; v++) {  // every maxiTrigger: previousValue = 1, firstTrigger = 1; maxiStep::first = true
            if (kind == MXG_SEQ_COUNTER) { d[V + v] = d[2 * V + v] = 1.0; i[v] = i[V + v] = 1; }
            else { d[v] = 1.0; i[v] = 1; if (kind == MXG_SEQ_STEP) i[V + v] = 1; }
        }
        dst_.upload(d); ist_.upload(i);
    }
    void run(size_t N, const double *a, const double *b, const double *par, double *out, void *stream) {
        check(mxg_seq_signal(kind_, V, N, a, b, val_.tab(), val_.len(), val_.P, val_.L, has_vsel_ ? vsel_.get() : nullptr, par, dst_.get(),
                             ist_.get(), out, stream), "mxg_seq_signal");
    }
    int kind_;
    size_t V;
    SeqTable val_;
    DeviceArray<double> dst_;
    DeviceArray<int64_t> ist_;
    DeviceArray<int32_t> vsel_;
    bool has_vsel_ = false;
};
}  // namespace maxigpu

class maxiTriggerBank : public maxigpu::SeqSignalBank {  // maxiTrigger::onZX
public:
    explicit maxiTriggerBank(size_t voices) : SeqSignalBank(MXG_SEQ_ONZX, voices) {}
    void onZX(size_t N, const double *d_in, double *d_out, void *stream = nullptr) { run(N, d_in, nullptr, nullptr, d_out, stream); }
};
class maxiCounterBank : public maxigpu::SeqSignalBank {  // maxiCounter::count
public:
    explicit maxiCounterBank(size_t voices) : SeqSignalBank(MXG_SEQ_COUNTER, voices) {}
    void count(size_t N, const double *d_inc, const double *d_reset, double *d_out, void *stream = nullptr) {
        run(N, d_inc, d_reset, nullptr, d_out, stream);
    }
};
class maxiStepBank : public maxigpu::SeqSignalBank {  // maxiStep::pull; d_step [V] (null = 1)
public:
    maxiStepBank(size_t voices, const std::vector<std::vector<double>> &values) : SeqSignalBank(MXG_SEQ_STEP, voices) { setValues(values); }
    void pull(size_t N, const double *d_trig, const double *d_step, double *d_out, void *stream = nullptr) {
        run(N, d_trig, nullptr, d_step, d_out, stream);
    }
};
class maxiIndexBank : public maxigpu::SeqSignalBank {  // maxiIndex::pull
public:
    maxiIndexBank(size_t voices, const std::vector<std::vector<double>> &values) : SeqSignalBank(MXG_SEQ_INDEX, voices) { setValues(values); }
    void pull(size_t N, const double *d_trig, const double *d_index, double *d_out, void *stream = nullptr) {
        run(N, d_trig, d_index, nullptr, d_out, stream);
    }
};
class maxiZXToPulseBank : public maxigpu::SeqSignalBank {  // maxiZXToPulse::play; d_hold [V] samples (null = 0)
public:
    explicit maxiZXToPulseBank(size_t voices) : SeqSignalBank(MXG_SEQ_ZXTOPULSE, voices) {}
    void play(size_t N, const double *d_in, const double *d_hold, double *d_out, void *stream = nullptr) {
        run(N, d_in, nullptr, d_hold, d_out, stream);
    }
};

// ---- maxiSample play family (H:602-783): V play heads over one sample ---------------------------------------
class maxiSampleBank {
public:
    explicit maxiSampleBank(size_t voices)
        : V(voices), position_(voices), a_(voices), start_(voices), end_(voices), zxPrev_(voices), phasorPrev_(voices),
          zxFirst_(voices), phasorFirst_(voices) {
        zxPrev_.upload(std::vector<double>(V, 1.0));     // maxiTrigger::previousValue = 1, firstTrigger = 1 (H:593-594)
        zxFirst_.upload(std::vector<int32_t>(V, 1));
        phasorFirst_.upload(std::vector<int32_t>(V, 1));  // phasorFirst = 1, phasorPrev = 0 (H:731-732)
    }
    ~maxiSampleBank() { clear(); }
    maxiSampleBank(const maxiSampleBank &) = delete;
    maxiSampleBank &operator=(const maxiSampleBank &) = delete;
    void setSample(const std::vector<double> &sampleData) {  // H:670-678
        clear();
        d_samples_ = mxg_sample_upload(sampleData.data(), sampleData.size());
        if (!d_samples_) throw std::runtime_error(std::string("mxg_sample_upload: ") + mxg_last_error());
        length_ = sampleData.size();
        mySampleRate = 44100;
        position_.upload(std::vector<double>(V, (double)length_ - 1));
    }
    void setSampleAndRate(const std::vector<double> &sampleData, int sampleRate) { setSample(sampleData); mySampleRate = sampleRate; }
    // load(fileName, channel) C:605-692: 16-bit PCM WAV, de-interleaved and normalised on the device; position = size (C:681)
    bool load(const std::string &fileName, int channel = 0) {
        size_t n = 0;
        double *p = mxg_sample_load_wav(fileName.c_str(), channel, &n, wavHeader_);
        if (!p) return false;  // the reference's `result`
        clear();
        d_samples_ = p;
        length_ = n;
        mySampleRate = wavHeader_[4];
        position_.upload(std::vector<double>(V, (double)n));
        return true;
    }
    bool save(const std::string &fileName) {  // C:698-725
        return mxg_sample_save_wav(fileName.c_str(), d_samples_, length_, wavHeader_, nullptr) == MXG_OK;
    }
    void trigger() { position_.upload(std::vector<double>(V, 0.0)); }  // C:597-600
    void setPositions(const std::vector<double> &p) { position_.upload(p); }
    void setSpeeds(const std::vector<double> &a) { a_.upload(a); }
    void setStartEnd(const std::vector<double> &s, const std::vector<double> &e) { start_.upload(s); end_.upload(e); }
    size_t getLength() const { return length_; }
    bool isReady() const { return length_ > 1; }
    const double *deviceSamples() const { return d_samples_; }
    std::vector<double> download() const {  // the buffer as the reference's public `amplitudes` would hold it
        std::vector<double> h(length_);
        if (length_) maxigpu::check(mxg_memcpy_d2h(h.data(), d_samples_, sizeof(double) * length_, nullptr), "mxg_memcpy_d2h");
        return h;
    }
    void clear() { if (d_samples_) mxg_sample_free(d_samples_); d_samples_ = nullptr; length_ = 0; }
    void render(int mode, size_t N, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_sample_render(mode, V, N, d_samples_, length_, mySampleRate, a_.get(), 0, start_.get(), end_.get(),
                                         position_.get(), d_out, stream), "mxg_sample_render");
    }
    void play(size_t N, double *d_out) { render(MXG_SMP_PLAY, N, d_out); }
    void playOnce(size_t N, double *d_out) { render(MXG_SMP_PLAYONCE, N, d_out); }
    void playAtSpeed(size_t N, double *d_out) { render(MXG_SMP_PLAYATSPEED, N, d_out); }
    // trigger-driven players (C:1006-1042): d_trig [N][V]; speed = setSpeeds(), offset/length (or pos) = setStartEnd()
    void renderTrig(int mode, size_t N, const double *d_trig, double *d_out, void *stream = nullptr) {
        const bool ph = mode == MXG_SMP_PLAYWITHPHASOR;
        maxigpu::check(mxg_sample_render_trig(mode, V, N, d_samples_, length_, mySampleRate, d_trig, a_.get(), 0, start_.get(),
                                              end_.get(), position_.get(), ph ? phasorPrev_.get() : zxPrev_.get(),
                                              ph ? phasorFirst_.get() : zxFirst_.get(), d_out, stream), "mxg_sample_render_trig");
    }
    void playOnZX(size_t N, const double *d_trig, double *d_out) { renderTrig(MXG_SMP_PLAYONZX, N, d_trig, d_out); }
    void playOnZXAtSpeed(size_t N, const double *d_trig, double *d_out) { renderTrig(MXG_SMP_PLAYONZXATSPEED, N, d_trig, d_out); }
    void playOnZXAtSpeedFromOffset(size_t N, const double *d_trig, double *d_out) { renderTrig(MXG_SMP_PLAYONZXATSPEEDFROMOFFSET, N, d_trig, d_out); }
    void playOnZXAtSpeedBetweenPoints(size_t N, const double *d_trig, double *d_out) { renderTrig(MXG_SMP_PLAYONZXATSPEEDBETWEENPOINTS, N, d_trig, d_out); }
    void loopSetPosOnZX(size_t N, const double *d_trig, double *d_out) { renderTrig(MXG_SMP_LOOPSETPOSONZX, N, d_trig, d_out); }
    void playWithPhasor(size_t N, const double *d_pha, double *d_out) { renderTrig(MXG_SMP_PLAYWITHPHASOR, N, d_pha, d_out); }  // C:753-816
    int mySampleRate = 44100;

private:
    size_t V;
    double *d_samples_ = nullptr;
    size_t length_ = 0;
    int32_t wavHeader_[8] = {36, 16, 1, 1, 44100, 88200, 2, 16};  // ChunkSize .. BitsPerSample of the last load()
    maxigpu::DeviceArray<double> position_, a_, start_, end_, zxPrev_, phasorPrev_;
    maxigpu::DeviceArray<int32_t> zxFirst_, phasorFirst_;
};

// ---- maxiFFT / maxiMFCC batches (L/maxiFFT.h, L/maxiMFCC.h) ----------------------------------------------------
class maxiFFTBatch {
public:
    enum fftModes { NO_POLAR_CONVERSION = 0, WITH_POLAR_CONVERSION = 1 };
    ~maxiFFTBatch() { if (plan_) mxg_fft_plan_destroy(plan_); }
    void setup(int fftSize = 1024, int hopSize = 512, int windowSize = 0) {  // L/maxiFFT.cpp:45-60
        if (plan_) mxg_fft_plan_destroy(plan_);
        maxigpu::check(mxg_init(-1), "mxg_init");
        plan_ = mxg_fft_plan_create(fftSize, hopSize, windowSize);
        if (!plan_) throw std::runtime_error(std::string("mxg_fft_plan_create: ") + mxg_last_error());
        fftSize_ = fftSize; hopSize_ = hopSize; bins_ = fftSize / 2;
    }
    int getNumBins() const { return bins_; }
    int getFFTSize() const { return fftSize_; }
    int getHopSize() const { return hopSize_; }
    // frames every `frame_stride` samples of a device signal -> [nframes][bins] outputs (any may be null)
    void process(const float *d_signal, size_t frame_stride, size_t nframes, float *d_mags, float *d_phases,
                 float *d_real = nullptr, float *d_imag = nullptr, void *stream = nullptr) {
        maxigpu::check(mxg_fft_batch(plan_, d_signal, frame_stride, nframes, d_real, d_imag, d_mags, d_phases, stream), "mxg_fft_batch");
    }
    // magsToDB / spectralFlatness / spectralCentroid (L/maxiFFT.cpp:101-132) for every frame; any output may be null
    void features(const float *d_mags, size_t nframes, float *d_db, float *d_flatness, float *d_centroid, void *stream = nullptr) {
        maxigpu::check(mxg_fft_features(plan_, d_mags, nframes, d_db, d_flatness, d_centroid, stream), "mxg_fft_features");
    }

private:
    mxg_fft_plan *plan_ = nullptr;
    int fftSize_ = 0, hopSize_ = 0, bins_ = 0;
};

// maxiIFFT (L/maxiFFT.h:117-156), SPECTRUM mode, over batches of spectra; the overlap-add buffer is carried
class maxiIFFTBatch {
public:
    ~maxiIFFTBatch() { if (plan_) mxg_ifft_plan_destroy(plan_); }
    void setup(int fftSize = 1024, int hopSize = 512, int windowSize = 0) {  // L/maxiFFT.cpp:140-153
        if (plan_) mxg_ifft_plan_destroy(plan_);
        maxigpu::check(mxg_init(-1), "mxg_init");
        plan_ = mxg_ifft_plan_create(fftSize, hopSize, windowSize);
        if (!plan_) throw std::runtime_error(std::string("mxg_ifft_plan_create: ") + mxg_last_error());
        fftSize_ = fftSize; hopSize_ = hopSize;
        buffer_.resize((size_t)fftSize);  // zero-filled, as setup() leaves `buffer`
    }
    int getNumBins() const { return fftSize_ / 2; }
    // d_mags/d_phases [nframes][bins] -> d_signal [nframes*hopSize]: what process() returns, hopSize calls per spectrum
    void process(const float *d_mags, const float *d_phases, size_t nframes, float *d_signal, void *stream = nullptr) {
        maxigpu::check(mxg_ifft_batch(plan_, d_mags, d_phases, nframes, buffer_.get(), d_signal, nullptr, stream), "mxg_ifft_batch");
    }

private:
    mxg_ifft_plan *plan_ = nullptr;
    int fftSize_ = 0, hopSize_ = 0;
    maxigpu::DeviceArray<float> buffer_;
};

// V maxiFFT objects after setup(fftSize, hopSize, windowSize), fed in lock-step with what a bank rendered: double [N][V], any N,
// any split into calls (mxg_fft_bank_*, kernel K29).  A call returns frames(N) frames per stream.
class maxiFFTBank {
public:
    enum Layout { FRAME_MAJOR = 0, STREAM_MAJOR = 1 };  // row = f * V + v | row = v * F + f
    maxiFFTBank(size_t V, int fftSize = 1024, int hopSize = 512, int windowSize = 0)
        : V_(V), fftSize_(fftSize), hopSize_(hopSize), windowSize_(windowSize) {
        h_ = mxg_fft_bank_create(V, fftSize, hopSize, windowSize);
        if (!h_) throw std::runtime_error(std::string("mxg_fft_bank_create: ") + mxg_last_error());
    }
    maxiFFTBank(const maxiFFTBank &) = delete;
    maxiFFTBank &operator=(const maxiFFTBank &) = delete;
    ~maxiFFTBank() { mxg_fft_bank_destroy(h_); }
    size_t voices() const { return V_; }
    int getNumBins() const { return fftSize_ / 2; }
    int pos() const { return mxg_fft_bank_pos(h_); }
    // frames every stream completes inside the next call of N samples
    size_t frames(size_t N) const {
        size_t F = 0;
        maxigpu::check(mxg_spectral_bank_plan_host(fftSize_, hopSize_, windowSize_, pos(), 0, N, &F, nullptr, nullptr, nullptr, nullptr),
                       "mxg_spectral_bank_plan_host");
        return F;
    }
    // d_in [N][V] -> fp32 [V * frames(N)][bins] outputs (any may be null, not all)
    void process(const double *d_in, size_t N, float *d_mags, float *d_phases, float *d_real = nullptr, float *d_imag = nullptr,
                 Layout layout = FRAME_MAJOR, void *stream = nullptr) {
        maxigpu::check(mxg_fft_bank_process(h_, d_in, N, (int)layout, d_real, d_imag, d_mags, d_phases, stream), "mxg_fft_bank_process");
    }
    void reset() { maxigpu::check(mxg_fft_bank_reset(h_), "mxg_fft_bank_reset"); }

private:
    mxg_fft_bank *h_ = nullptr;
    size_t V_;
    int fftSize_, hopSize_, windowSize_;
};

// V maxiIFFT objects after setup(fftSize, hopSize, windowSize), called once per sample: rows of spectra -> double [N][V]
// (mxg_ifft_bank_*, kernel K29).  DIRECT rows: one per consumption point, rows(N) of them.  AFTER_FFT rows: what a maxiFFTBank of
// the same hop, created at the same time, returned for the same N -- the loop of ffttest.cpp, the last frame held across calls.
class maxiIFFTBank {
public:
    enum Form { SPECTRUM = 0, CARTESIAN = 1 };
    enum Rows { DIRECT = 0, AFTER_FFT = 1 };
    maxiIFFTBank(size_t V, int fftSize = 1024, int hopSize = 512, int windowSize = 0) : V_(V), fftSize_(fftSize), hopSize_(hopSize) {
        h_ = mxg_ifft_bank_create(V, fftSize, hopSize, windowSize);
        if (!h_) throw std::runtime_error(std::string("mxg_ifft_bank_create: ") + mxg_last_error());
    }
    maxiIFFTBank(const maxiIFFTBank &) = delete;
    maxiIFFTBank &operator=(const maxiIFFTBank &) = delete;
    ~maxiIFFTBank() { mxg_ifft_bank_destroy(h_); }
    size_t voices() const { return V_; }
    int getNumBins() const { return fftSize_ / 2; }
    int pos() const { return mxg_ifft_bank_pos(h_); }
    // rows per stream the next call of N samples takes
    size_t rows(size_t N, Rows mode = DIRECT) const {
        size_t F = 0, C = 0;
        maxigpu::check(mxg_spectral_bank_plan_host(fftSize_, hopSize_, 0, pos(), pos(), N, &F, &C, nullptr, nullptr, nullptr),
                       "mxg_spectral_bank_plan_host");
        return mode == AFTER_FFT ? F : C;
    }
    // d_a / d_b fp32 [V * rows(N, mode)][bins] (magnitudes / phases, or real / imag) -> d_out [N][V]
    void process(const float *d_a, const float *d_b, size_t N, double *d_out, Form form = SPECTRUM, Rows mode = DIRECT,
                 maxiFFTBank::Layout layout = maxiFFTBank::FRAME_MAJOR, void *stream = nullptr) {
        maxigpu::check(mxg_ifft_bank_process(h_, (int)form, (int)mode, (int)layout, d_a, d_b, rows(N, mode), N, d_out, stream),
                       "mxg_ifft_bank_process");
    }
    const float *buffers() const { return mxg_ifft_bank_buffer(h_); }  // device [V][fftSize]
    void reset() { maxigpu::check(mxg_ifft_bank_reset(h_), "mxg_ifft_bank_reset"); }

private:
    mxg_ifft_bank *h_ = nullptr;
    size_t V_;
    int fftSize_, hopSize_;
};

class maxiMFCCBatch {
public:
    ~maxiMFCCBatch() { if (plan_) mxg_mfcc_plan_destroy(plan_); }
    void setup(unsigned numBins, unsigned numFilters, unsigned numCoeffs, double minFreq, double maxFreq) {  // L/maxiMFCC.h:56-75
        if (plan_) mxg_mfcc_plan_destroy(plan_);
        plan_ = mxg_mfcc_plan_create(numBins, numFilters, numCoeffs, minFreq, maxFreq);
        if (!plan_) throw std::runtime_error(std::string("mxg_mfcc_plan_create: ") + mxg_last_error());
        numBins_ = numBins;
    }
    void mfcc(const float *d_mags, size_t nframes, double *d_mfcc, int method = 0, void *stream = nullptr) {  // L/maxiMFCC.h:77-81
        maxigpu::check(mxg_mfcc_batch(plan_, d_mags, numBins_, nframes, nullptr, nullptr, d_mfcc, method, stream), "mxg_mfcc_batch");
    }

private:
    mxg_mfcc_plan *plan_ = nullptr;
    unsigned numBins_ = 0;
};

// ---- maxiBark / maxiFFTOctaveAnalyzer over batches of magnitude rows (K19) ---------------------------------------------------
class maxiBarkBatch {
public:
    ~maxiBarkBatch() { if (plan_) mxg_bark_plan_destroy(plan_); }
    void setup(unsigned sampleRate, unsigned bufferSize) {  // L/maxiBark.h:40-62
        if (plan_) mxg_bark_plan_destroy(plan_);
        plan_ = mxg_bark_plan_create(sampleRate, bufferSize);
        if (!plan_) throw std::runtime_error(std::string("mxg_bark_plan_create: ") + mxg_last_error());
        specSize_ = bufferSize / 2;
    }
    std::vector<int> limits() const {
        std::vector<int> lim(MXG_BARK_BANDS + 1);
        maxigpu::check(mxg_bark_plan_limits(plan_, lim.data()), "mxg_bark_plan_limits");
        return lim;
    }
    // d_spectrum [nframes][bufferSize / 2] -> any of d_specific / d_relative [nframes][24], d_total [nframes], d_bandsum (null: not produced)
    void analyse(const float *d_spectrum, size_t nframes, double *d_specific, double *d_relative = nullptr, double *d_total = nullptr,
                 double *d_bandsum = nullptr, void *stream = nullptr) {
        maxigpu::check(mxg_bark_batch(plan_, d_spectrum, specSize_, nframes, d_bandsum, d_specific, d_relative, d_total, stream), "mxg_bark_batch");
    }

private:
    mxg_bark_plan *plan_ = nullptr;
    unsigned specSize_ = 0;
};

class maxiOctaveBatch {
public:
    int peakHoldTime = 0;            // L/maxiFFT.cpp:255-258
    float peakDecayRate = 0.9f, linearEQIntercept = 1.0f, linearEQSlope = 0.0f;
    explicit maxiOctaveBatch(size_t streams = 1) : S(streams) {}
    ~maxiOctaveBatch() { if (plan_) mxg_octave_plan_destroy(plan_); }
    void setup(float samplingRate, int nSpectrum, int nAveragesPerOctave) {  // L/maxiFFT.cpp:207-259; peaks and hold counters start at 0
        if (plan_) mxg_octave_plan_destroy(plan_);
        plan_ = mxg_octave_plan_create(samplingRate, nSpectrum, nAveragesPerOctave);
        if (!plan_) throw std::runtime_error(std::string("mxg_octave_plan_create: ") + mxg_last_error());
        nSpectrum_ = nSpectrum;
        nAverages_ = mxg_octave_plan_averages(plan_);
        peaks_ = maxigpu::DeviceArray<float>(S * (size_t)nAverages_);
        hold_ = maxigpu::DeviceArray<int32_t>(S * (size_t)nAverages_);
    }
    int nAverages() const { return nAverages_; }
    // d_mags [streams * frames][nSpectrum], stream-major -> d_averages and (optional) d_peaks [streams * frames][nAverages]
    void calculate(const float *d_mags, size_t frames, float *d_averages, float *d_peaks = nullptr, void *stream = nullptr) {
        maxigpu::check(mxg_octave_batch(plan_, d_mags, (size_t)nSpectrum_, S, frames, linearEQIntercept, linearEQSlope, peakHoldTime, peakDecayRate,
                                        d_averages, d_peaks, peaks_.get(), hold_.get(), stream), "mxg_octave_batch");
    }
    const size_t S;

private:
    mxg_octave_plan *plan_ = nullptr;
    int nSpectrum_ = 0, nAverages_ = 0;
    maxigpu::DeviceArray<float> peaks_;
    maxigpu::DeviceArray<int32_t> hold_;
};

// ---- maxiTimeStretch / maxiStretch banks (L/maxiGrains.h) ---------------------------------------------------------
class maxiTimeStretchBank {
public:
    maxiTimeStretchBank(size_t streams, maxiSampleBank *sample, int window_kind = 0)
        : S(streams), sample_(sample), window_(window_kind), st_(4 * streams), gst_(32 * streams), speed_(streams) {}
    ~maxiTimeStretchBank() { if (plan_) mxg_grain_plan_destroy(plan_); }
    void setPosition(const std::vector<double> &pos01) {  // L/maxiGrains.h:335-338
        std::vector<double> st = st_.download();
        const double len = (double)sample_->getLength();
        for (size_t s = 0; s < S; s++) {
            double p = pos01[s] * len;
            st[s] = p < 0 ? 0 : (p > len - 1 ? len - 1 : p);
        }
        st_.upload(st);
    }
    void setSpeeds(const std::vector<double> &speed) { speed_.upload(speed); }
    // play(speed, grainLength, overlaps) for N samples of every stream -> d_out [N][S]
    void play(double grainLength, int overlaps, size_t N, double *d_out, void *stream = nullptr) {
        plan(grainLength);
        maxigpu::check(mxg_granular_render(plan_, mode_, S, N, sample_->deviceSamples(), sample_->getLength(), overlaps, speed_.get(),
                                           nullptr, nullptr, nullptr, 0, st_.get(), gst_.get(), d_out, stream), "mxg_granular_render");
    }
    // playAtPosition(pos, grainLength, overlaps) (L/maxiGrains.h:359-367): d_pos = the per-sample [N][S] position signal
    void playAtPosition(const double *d_pos, double grainLength, int overlaps, size_t N, double *d_out, void *stream = nullptr) {
        plan(grainLength);
        maxigpu::check(mxg_granular_render(plan_, 2, S, N, sample_->deviceSamples(), sample_->getLength(), overlaps, d_pos, nullptr,
                                           nullptr, nullptr, 0, st_.get(), gst_.get(), d_out, stream), "mxg_granular_render");
    }

protected:
    int mode_ = 0;
    mxg_grain_plan *plan_handle() const { return plan_; }
    const double *speeds() const { return speed_.get(); }
    double *state() { return st_.get(); }
    double *grains() { return gst_.get(); }
    void plan(double grainLength) {
        if (!plan_ || grainLength != grainLength_) {
            if (plan_) mxg_grain_plan_destroy(plan_);
            plan_ = mxg_grain_plan_create(window_, grainLength, sample_->mySampleRate);
            if (!plan_) throw std::runtime_error(std::string("mxg_grain_plan_create: ") + mxg_last_error());
            grainLength_ = grainLength;
        }
    }

private:
    size_t S;
    maxiSampleBank *sample_;
    int window_;
    mxg_grain_plan *plan_ = nullptr;
    double grainLength_ = 0;
    maxigpu::DeviceArray<double> st_, gst_, speed_;
};

// ---- maxiPitchShift bank (L/maxiGrains.h:374-432): same grains, speed uncoupled from position ----------------------
class maxiPitchShiftBank : public maxiTimeStretchBank {
public:
    maxiPitchShiftBank(size_t streams, maxiSampleBank *sample, int window_kind = 0)
        : maxiTimeStretchBank(streams, sample, window_kind) { mode_ = 3; }
};

// ---- maxiStretch bank (L/maxiGrains.h:437-542): pitch (grain speed) and time stretch uncoupled, the default loop ----------
class maxiStretchBank : public maxiTimeStretchBank {
public:
    maxiStretchBank(size_t streams, maxiSampleBank *sample, int window_kind = 0)
        : maxiTimeStretchBank(streams, sample, window_kind), nS_(streams), smp_(sample), rate_(streams) { mode_ = 1; }
    void setPitch(const std::vector<double> &pitchstretch) { setSpeeds(pitchstretch); }  // the first argument of play()
    void setRate(const std::vector<double> &timestretch) { rate_.upload(timestretch); }   // the second
    // play(pitchstretch, timestretch, grainLength, overlaps) for N samples of every stream -> d_out [N][S]; d_rnd (optional):
    // int32 [S][R], the values rand() % 10 returns at the spawns of each stream (NULL: 0, no jitter)
    void play(double grainLength, int overlaps, size_t N, double *d_out, const int32_t *d_rnd = nullptr, size_t R = 0,
              void *stream = nullptr) {
        plan(grainLength);
        maxigpu::check(mxg_granular_render(plan_handle(), 1, nS_, N, smp_->deviceSamples(), smp_->getLength(), overlaps, speeds(),
                                           rate_.get(), nullptr, d_rnd, R, state(), grains(), d_out, stream), "mxg_granular_render");
    }

private:
    size_t nS_;
    maxiSampleBank *smp_;
    maxigpu::DeviceArray<double> rate_;
};

// ---- maxiConvolve (L/maxiConvolve.h:19-34, maxiConvolve.cpp:13-107), block form --------------------------------------------
// setup() analyses the impulse (a maxiSampleBank's buffer, its play head where load() left it); play() takes nblocks * fftsize
// input samples at once.  as_intended = false reproduces what the reference computes (its COMPLEX-mode inverse never receives the
// sums: silence after the window), true what it was written to do; both bit-exact (include/maxigpu.h, mxg_convolve_play).
class maxiConvolveBlock {
public:
    ~maxiConvolveBlock() { if (c_) mxg_convolve_destroy(c_); }
    void setup(const std::vector<double> &impulse, double position0, int fftsize = 1024, int hopsize = 256) {
        if (c_) mxg_convolve_destroy(c_);
        c_ = mxg_convolve_create(impulse.data(), impulse.size(), position0, fftsize, hopsize);
        if (!c_) throw std::runtime_error(std::string("mxg_convolve_create: ") + mxg_last_error());
        fftsize_ = fftsize;
    }
    int frames() const { return c_ ? mxg_convolve_frames(c_) : 0; }
    int fftSize() const { return fftsize_; }
    void play(const float *d_in, size_t nblocks, float *d_out, bool as_intended = false, void *stream = nullptr) {
        maxigpu::check(mxg_convolve_play(c_, d_in, nblocks, d_out, as_intended ? 1 : 0, stream), "mxg_convolve_play");
    }
    void reset() { maxigpu::check(mxg_convolve_reset(c_), "mxg_convolve_reset"); }

private:
    mxg_convolve *c_ = nullptr;
    int fftsize_ = 0;
};

// ---- maxiConvolveBank: V maxiConvolve objects over shared impulses (include/maxigpu.h, mxg_convolve_bank_*; kernel K24) ----------
// impulses[i] = the amplitudes of impulse i (its play head where load() leaves it: at its size), imp_of[v] = the impulse of stream v.
// play(): float [V][nblocks * fftsize] in and out; play_nv(): the other banks' double [N][V] blocks, N = nblocks * fftsize (an
// oscillator bank's output goes in, a maxiMixBank takes what comes out).  Stream v is bit for bit a maxiConvolveBlock of its own.
class maxiConvolveBank {
public:
    maxiConvolveBank(size_t V, const std::vector<std::vector<double>> &impulses, const std::vector<int> &imp_of, int fftsize = 1024,
                     int hopsize = 256)
        : V_(V), fftsize_(fftsize) {
        std::vector<const double *> amps;
        std::vector<size_t> lens;
        std::vector<double> pos0;
        for (const std::vector<double> &a : impulses) {
            amps.push_back(a.data());
            lens.push_back(a.size());
            pos0.push_back((double)a.size());
        }
        if (imp_of.size() != V) throw std::runtime_error("maxiConvolveBank: imp_of needs one entry per stream");
        b_ = mxg_convolve_bank_create(V, impulses.size(), amps.data(), lens.data(), pos0.data(), imp_of.data(), fftsize, hopsize);
        if (!b_) throw std::runtime_error(std::string("mxg_convolve_bank_create: ") + mxg_last_error());
    }
    ~maxiConvolveBank() { if (b_) mxg_convolve_bank_destroy(b_); }
    maxiConvolveBank(const maxiConvolveBank &) = delete;
    maxiConvolveBank &operator=(const maxiConvolveBank &) = delete;
    size_t size() const { return V_; }
    int fftSize() const { return fftsize_; }
    int frames(size_t i) const { return mxg_convolve_bank_frames(b_, i); }
    void play(const float *d_in, size_t nblocks, float *d_out, bool as_intended = false, void *stream = nullptr) {
        maxigpu::check(mxg_convolve_bank_play(b_, d_in, nblocks, d_out, as_intended ? 1 : 0, stream), "mxg_convolve_bank_play");
    }
    void play_nv(const double *d_in, size_t nblocks, double *d_out, bool as_intended = false, void *stream = nullptr) {
        maxigpu::check(mxg_convolve_bank_play_nv(b_, d_in, nblocks, d_out, as_intended ? 1 : 0, stream), "mxg_convolve_bank_play_nv");
    }
    void reset() { maxigpu::check(mxg_convolve_bank_reset(b_), "mxg_convolve_bank_reset"); }

private:
    size_t V_;
    int fftsize_;
    mxg_convolve_bank *b_ = nullptr;
};

// ---- maxiSampler banks (L/maxiSynths.h:137-187, maxiSynths.cpp:262-491) ------------------------------------------------------
// NS samplers of `voices` slots each over one sample; the control methods edit host copies of the slot state between renders,
// exactly as the reference's methods edit its members; play(N) renders N calls of maxiSampler::play() for every sampler.
class maxiSamplerBank {
public:
    maxiSamplerBank(size_t samplers, int voices, maxiSampleBank *sample)
        : NS(samplers), voices_(voices), V(samplers * (size_t)voices), sample_(sample), pitch_(V, 0.0), gain_(V, 0.0), par_(4 * V),
          hold_(V, 1), position_(V, 0.0), trig_(V, 0), outhold_(V, 0.0), dst_(2 * V, 0.0), ist_(6 * V, 0), currentVoice_(samplers, 0),
          d_freq_(V), d_gain_(V), d_par_(4 * V), d_hold_(V), d_pos_(V), d_trig_(V), d_outhold_(V), d_dst_(2 * V), d_ist_(6 * V) {
        for (size_t v = 0; v < V; v++) {  // ctor, maxiSynths.cpp:262-283
            par_[0 * V + v] = mxg_env_coeff_host(0, 0);
            par_[1 * V + v] = mxg_env_coeff_host(1, 1);
            par_[2 * V + v] = 1.;
            par_[3 * V + v] = mxg_env_coeff_host(2, 2000);
            position_[v] = (double)sample->getLength();  // after load(); setSample leaves len - 1: use resetPositions()
        }
    }
    bool sustain = true;
    void resetPositions(double p) { pull(); std::fill(position_.begin(), position_.end(), p); dirty_ = true; }
    void setPitch(size_t sampler, double pitchIn, bool setall = false) { for (size_t v : slots(sampler, setall)) pitch_[v] = pitchIn; }
    void midiNoteOn(size_t sampler, double pitchIn, double velocity, bool setall = false) {  // :341-358
        for (size_t v : slots(sampler, setall)) {
            pitch_[v] = pitchIn;
            if (!setall) gain_[v] = velocity / 128;
        }
    }
    void midiNoteOff(size_t sampler, double pitchIn) {  // :360-372
        pull();
        for (int i = 0; i < voices_; i++)
            if (pitch_[sampler * voices_ + i] == pitchIn) trig_[sampler * voices_ + i] = 0;
        dirty_ = true;
    }
    void setEnvelope(size_t sampler, int which /*0 attack 1 decay 2 sustain 3 release*/, double value, bool setall = true) {
        const double c = which == 2 ? value : mxg_env_coeff_host(which == 3 ? 2 : which, value);
        for (size_t v : slots(sampler, setall)) par_[(size_t)which * V + v] = c;
    }
    void trigger(size_t sampler) {  // :484-491
        pull();
        const size_t v = sampler * voices_ + (size_t)currentVoice_[sampler];
        trig_[v] = 1;
        position_[v] = 0;
        currentVoice_[sampler] = (currentVoice_[sampler] + 1) % voices_;
        dirty_ = true;
    }
    // N calls of play() for every sampler -> d_mix [N][NS]
    void play(size_t N, double *d_mix, void *stream = nullptr) {
        if (dirty_) {
            d_pos_.upload(position_); d_trig_.upload(trig_); d_outhold_.upload(outhold_); d_dst_.upload(dst_); d_ist_.upload(ist_);
            dirty_ = false;
        }
        std::vector<double> freq(V);
        maxigpu::check(mxg_sampler_freq_host(V, pitch_.data(), sample_->getLength(), freq.data()), "mxg_sampler_freq_host");
        d_freq_.upload(freq); d_gain_.upload(gain_); d_par_.upload(par_); d_hold_.upload(hold_);
        maxigpu::check(mxg_sampler_render(V, N, voices_, sustain ? 1 : 0, sample_->deviceSamples(), sample_->getLength(), d_freq_.get(),
                                          d_gain_.get(), d_par_.get(), d_hold_.get(), d_pos_.get(), d_trig_.get(), d_outhold_.get(),
                                          d_dst_.get(), d_ist_.get(), d_mix, nullptr, stream), "mxg_sampler_render");
        fresh_ = false;
    }

private:
    size_t NS;
    int voices_;
    size_t V;
    maxiSampleBank *sample_;
    std::vector<double> pitch_, gain_, par_;
    std::vector<int64_t> hold_;
    std::vector<double> position_;
    std::vector<int32_t> trig_;
    std::vector<double> outhold_, dst_;
    std::vector<int64_t> ist_;
    std::vector<int> currentVoice_;
    maxigpu::DeviceArray<double> d_freq_, d_gain_, d_par_;
    maxigpu::DeviceArray<int64_t> d_hold_;
    maxigpu::DeviceArray<double> d_pos_;
    maxigpu::DeviceArray<int32_t> d_trig_;
    maxigpu::DeviceArray<double> d_outhold_, d_dst_;
    maxigpu::DeviceArray<int64_t> d_ist_;
    bool dirty_ = true, fresh_ = true;
    std::vector<size_t> slots(size_t sampler, bool setall) const {
        std::vector<size_t> r;
        if (setall) for (int i = 0; i < voices_; i++) r.push_back(sampler * voices_ + (size_t)i);
        else r.push_back(sampler * voices_ + (size_t)currentVoice_[sampler]);
        return r;
    }
    void pull() {  // the device state back to the host copies (after a render)
        if (dirty_ || fresh_) return;
        position_ = d_pos_.download(); trig_ = d_trig_.download(); outhold_ = d_outhold_.download();
        dst_ = d_dst_.download(); ist_ = d_ist_.download();
    }
};

// V (1 ... 4096) linear filters with block-constant coefficients over LONG signals, parallel in time (mxg_scan_long_render, K28):
// maxiDCBlocker, maxiSVF, maxiBiquad, maxiFilter::lores / hires or maxiLagExp, the signal [N][V] cut into chunks of 2048 samples
// that a scan joins.  A tolerance mode (maxigpu.h: SCAN_LONG_RTOL per kind), not bit-exact against the sequential banks.  The state
// rows are those of the sequential entry point of the kind ([3][V], [5][V] or [1][V]): state() / set_state() hand a stream over to
// one and back.  V = 1 filters a plain contiguous signal, e.g. maxiLooperBank::deviceSamples(r); d_out == d_in is allowed.
// LORES, HIRES and LAG banks also take coefficients that move every sample (mxg_scan_long_render_swept, K31): processSwept /
// hostSwept, on the same state; sweepCoefficients makes the [N][3][V] array from a cutoff and a resonance per sample.
class maxiLongScanBank {
public:
    enum Kind { DC = 0, SVF = 1, BIQUAD = 2, LORES = 3, HIRES = 4, LAG = 5 };
    maxiLongScanBank(size_t voices, Kind kind) : V(voices), kind_(kind) {
        maxigpu::check(mxg_init(-1), "mxg_init");
        d_st_.resize(state_rows() * V);
    }
    size_t voices() const { return V; }
    Kind kind() const { return kind_; }
    size_t coef_rows() const { return kind_ == DC ? 1 : kind_ == SVF ? 9 : kind_ == BIQUAD ? 5 : 2; }
    size_t state_rows() const { return kind_ <= BIQUAD ? 3 : kind_ == LAG ? 1 : 5; }
    void setDC(const std::vector<double> &R) { set(DC, need(R)); }
    void setSVF(const std::vector<double> &cutoff, const std::vector<double> &res, double lp, double bp, double hp, double notch) {
        std::vector<double> c(9 * V);
        maxigpu::check(mxg_svf_coeffs_host(V, need(cutoff).data(), need(res).data(), c.data()), "mxg_svf_coeffs_host");
        const double mix[4] = {lp, bp, hp, notch};
        for (size_t r = 0; r < 4; r++)
            for (size_t v = 0; v < V; v++) c[(5 + r) * V + v] = mix[r];
        set(SVF, c);
    }
    void setBiquad(const std::vector<int32_t> &type, const std::vector<double> &cutoff, const std::vector<double> &Q, const std::vector<double> &peakGain) {
        if (type.size() != V) throw std::invalid_argument("maxiLongScanBank: one value per voice");
        std::vector<double> c(5 * V);
        maxigpu::check(mxg_biquad_coeffs_host(V, type.data(), need(cutoff).data(), need(Q).data(), need(peakGain).data(), c.data()), "mxg_biquad_coeffs_host");
        set(BIQUAD, c);
    }
    void setLores(const std::vector<double> &cutoff, const std::vector<double> &res) { set(LORES, cr(cutoff, res)); }
    void setHires(const std::vector<double> &cutoff, const std::vector<double> &res) { set(HIRES, cr(cutoff, res)); }
    void setLag(const std::vector<double> &alpha) {  // maxiLagExp::init: alphaReciprocal = 1 - alpha
        std::vector<double> c(need(alpha));
        for (size_t v = 0; v < V; v++) c.push_back(1.0 - alpha[v]);
        set(LAG, c);
    }
    const std::vector<double> &coefficients() const { return coef_; }
    // N samples per voice, d_in / d_out [N][V] on the device
    void process(size_t N, const double *d_in, double *d_out, void *stream = nullptr) {
        if (coef_.empty()) throw std::logic_error("maxiLongScanBank: no coefficients set");
        maxigpu::check(mxg_scan_long_render((int)kind_, V, N, d_in, d_coef_.get(), d_st_.get(), d_out, stream), "mxg_scan_long_render");
    }
    // the host twin (the device's bits) on host arrays from the state `st` [state_rows()][V], which it advances
    void host(size_t N, const double *h_in, double *h_out, std::vector<double> &st) const {
        if (coef_.empty() || st.size() != state_rows() * V) throw std::logic_error("maxiLongScanBank::host: coefficients and a whole state array");
        maxigpu::check(mxg_scan_long_host((int)kind_, V, N, h_in, coef_.data(), st.data(), h_out), "mxg_scan_long_host");
    }
    // The same with the coefficients of every sample (mxg_scan_long_render_swept, K31; LORES, HIRES and LAG): d_coef_ps
    // [N][coef_rows][V] on the device, coef_rows 2 ... 8, rows 0-1 read.  Shares the bank's state with process(); needs no setter.
    void processSwept(size_t N, const double *d_in, const double *d_coef_ps, size_t coef_rows, double *d_out, void *stream = nullptr) {
        maxigpu::check(mxg_scan_long_render_swept((int)kind_, V, N, d_in, d_coef_ps, coef_rows, d_st_.get(), d_out, stream), "mxg_scan_long_render_swept");
    }
    // its host twin (the device's bits) on host arrays from the state `st` [state_rows()][V], which it advances
    void hostSwept(size_t N, const double *h_in, const double *h_coef_ps, size_t coef_rows, double *h_out, std::vector<double> &st) const {
        if (st.size() != state_rows() * V) throw std::logic_error("maxiLongScanBank::hostSwept: a whole state array");
        maxigpu::check(mxg_scan_long_swept_host((int)kind_, V, N, h_in, h_coef_ps, coef_rows, st.data(), h_out), "mxg_scan_long_swept_host");
    }
    // host [N][3][V] for LORES / HIRES from cutoff and res [N][V]: mxg_filter_coeffs_host per sample, rows c, r, 0 -- what
    // mxg_filter_render_coefs takes, and processSwept with coef_rows = 3
    static std::vector<double> sweepCoefficients(Kind kind, size_t N, size_t V, const std::vector<double> &cutoff, const std::vector<double> &res) {
        if (kind != LORES && kind != HIRES) throw std::invalid_argument("maxiLongScanBank::sweepCoefficients: LORES or HIRES");
        if (cutoff.size() != N * V || res.size() != N * V) throw std::invalid_argument("maxiLongScanBank::sweepCoefficients: cutoff and res are [N][V]");
        std::vector<double> c(3 * N * V);
        for (size_t n = 0; n < N; n++)
            maxigpu::check(mxg_filter_coeffs_host(0, V, cutoff.data() + n * V, res.data() + n * V, c.data() + n * 3 * V), "mxg_filter_coeffs_host");
        return c;
    }
    std::vector<double> state() const {
        maxigpu::check(mxg_sync(), "mxg_sync");
        return d_st_.download();
    }
    void set_state(const std::vector<double> &st) {
        if (st.size() != state_rows() * V) throw std::invalid_argument("maxiLongScanBank::set_state: [state_rows()][V] values");
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_st_.upload(st);
    }

private:
    const std::vector<double> &need(const std::vector<double> &a) const {
        if (a.size() != V) throw std::invalid_argument("maxiLongScanBank: one value per voice");
        return a;
    }
    std::vector<double> cr(const std::vector<double> &cutoff, const std::vector<double> &res) const {
        std::vector<double> c(3 * V);
        maxigpu::check(mxg_filter_coeffs_host(0, V, need(cutoff).data(), need(res).data(), c.data()), "mxg_filter_coeffs_host");  // (lores and hires share c, r)
        c.resize(2 * V);
        return c;
    }
    void set(Kind k, const std::vector<double> &c) {
        if (k != kind_) throw std::logic_error("maxiLongScanBank: this setter is of another kind");
        coef_ = c;
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_coef_.upload(coef_);
    }
    size_t V;
    Kind kind_;
    std::vector<double> coef_;
    maxigpu::DeviceArray<double> d_coef_, d_st_;
};
