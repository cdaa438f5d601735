// include/maxiSynths.h -- DROP-IN for the reference's polyphonic sampler maxiSampler (src/libs/maxiSynths.h:137-187,
// maxiSynths.cpp:262-491): up to 32 slots of maxiEnv::adsr x maxiSample::play4 over one sample, summed in slot order, one
// play() per sample, executed through the C-ABI's mxg_sampler_render (sampler.hip; bit-exact incl. the in-order sum).
//
// play() is served from blocks: as long as no control method is called (trigger, midiNoteOn / Off, setPitch, the envelope
// setters ...) the slot parameters cannot change, so a launch renders the next 1, 2, 4 ... 512 calls at once and play() reads them
// back; a control call first rewinds the sampler to the state it had at the current sample (the block is re-rendered from its
// start state up to there: same kernel, same bits), then edits that state on the host exactly as the reference's method does.
// Limits against the reference: every slot plays the SAME sample (load / setSample with setall, the reference's default; a
// per-slot load is refused with a printed error), and the unused members (LFO1-4, filters, distortion: never touched by maxiSampler::play) are absent.
#pragma once
#include "maximilian.h"

class maxiSampler {
    static constexpr int kMax = 32;
    struct State {
        double position[kMax], outhold[kMax], dst[2 * kMax];
        int32_t trig[kMax];
        int64_t ist[6 * kMax];
    };
    State cur_ = {}, end_ = {};
    double par_[4 * kMax], gain_[kMax];
    int64_t hold_[kMax];
    std::vector<double> blk_;
    size_t pos_ = 0, nextLen_ = 1;
    double *d_samples_ = nullptr;
    size_t len_ = 0;
    char *d_ = nullptr;  // device scratch, laid out in layout()
    bool dirty_ = true;  // parameters / state edited on the host since the last launch

    struct Lay { double *freq, *gain, *par, *pos, *outhold, *dst, *mix; int64_t *hold, *ist; int32_t *trig; };
    Lay layout() const {
        Lay l;
        double *p = reinterpret_cast<double *>(d_);
        l.freq = p; p += kMax;
        l.gain = p; p += kMax;
        l.par = p; p += 4 * kMax;
        l.pos = p; p += kMax;
        l.outhold = p; p += kMax;
        l.dst = p; p += 2 * kMax;
        l.mix = p; p += maxigpu::ps::kMaxBlock;
        l.hold = reinterpret_cast<int64_t *>(p); p += kMax;
        l.ist = reinterpret_cast<int64_t *>(p); p += 6 * kMax;
        l.trig = reinterpret_cast<int32_t *>(p);
        return l;
    }
    static constexpr size_t kBytes = sizeof(double) * (kMax * 10 + maxigpu::ps::kMaxBlock + kMax + 6 * kMax) + sizeof(int32_t) * kMax + 64;

    // state rows are [row][voices] on the device (V = voices): repack from the fixed-size host arrays
    void upload(const State &s) {
        MAXIGPU_TRY {
        using maxigpu::ps::check;
        const size_t V = (size_t)voices;
        if (!d_) {
            check(mxg_init(-1), "mxg_init");
            d_ = static_cast<char *>(mxg_malloc(kBytes));
            if (!d_) maxigpu::ps::fatal(std::string("mxg_malloc: ") + mxg_last_error());
        }
        const Lay l = layout();
        std::vector<double> dst(2 * V);
        std::vector<int64_t> ist(6 * V);
        for (size_t v = 0; v < V; v++) {
            for (int r = 0; r < 2; r++) dst[(size_t)r * V + v] = s.dst[r * kMax + (int)v];
            for (int r = 0; r < 6; r++) ist[(size_t)r * V + v] = s.ist[r * kMax + (int)v];
        }
        check(mxg_memcpy_h2d(l.pos, s.position, sizeof(double) * V, nullptr), "h2d");
        check(mxg_memcpy_h2d(l.outhold, s.outhold, sizeof(double) * V, nullptr), "h2d");
        check(mxg_memcpy_h2d(l.trig, s.trig, sizeof(int32_t) * V, nullptr), "h2d");
        check(mxg_memcpy_h2d(l.dst, dst.data(), sizeof(double) * 2 * V, nullptr), "h2d");
        check(mxg_memcpy_h2d(l.ist, ist.data(), sizeof(int64_t) * 6 * V, nullptr), "h2d");
        // parameters
        std::vector<double> par(4 * V), freq(V);
        for (size_t v = 0; v < V; v++)
            for (int r = 0; r < 4; r++) par[(size_t)r * V + v] = par_[r * kMax + (int)v];
        check(mxg_sampler_freq_host(V, pitch, len_, freq.data()), "mxg_sampler_freq_host");
        check(mxg_memcpy_h2d(l.freq, freq.data(), sizeof(double) * V, nullptr), "h2d");
        check(mxg_memcpy_h2d(l.gain, gain_, sizeof(double) * V, nullptr), "h2d");
        check(mxg_memcpy_h2d(l.par, par.data(), sizeof(double) * 4 * V, nullptr), "h2d");
        check(mxg_memcpy_h2d(l.hold, hold_, sizeof(int64_t) * V, nullptr), "h2d");
        }
        MAXIGPU_CATCH(return)
    }
    void download(State &s) {
        using maxigpu::ps::check;
        const size_t V = (size_t)voices;
        const Lay l = layout();
        std::vector<double> dst(2 * V);
        std::vector<int64_t> ist(6 * V);
        check(mxg_memcpy_d2h(s.position, l.pos, sizeof(double) * V, nullptr), "d2h");
        check(mxg_memcpy_d2h(s.outhold, l.outhold, sizeof(double) * V, nullptr), "d2h");
        check(mxg_memcpy_d2h(s.trig, l.trig, sizeof(int32_t) * V, nullptr), "d2h");
        check(mxg_memcpy_d2h(dst.data(), l.dst, sizeof(double) * 2 * V, nullptr), "d2h");
        check(mxg_memcpy_d2h(ist.data(), l.ist, sizeof(int64_t) * 6 * V, nullptr), "d2h");
        for (size_t v = 0; v < V; v++) {
            for (int r = 0; r < 2; r++) s.dst[r * kMax + (int)v] = dst[(size_t)r * V + v];
            for (int r = 0; r < 6; r++) s.ist[r * kMax + (int)v] = ist[(size_t)r * V + v];
        }
    }
    // render L calls of play() from cur_; leaves the state after them in end_ and the outputs in blk_
    void render(size_t L) {
        using maxigpu::ps::check;
        upload(cur_);
        const Lay l = layout();
        check(mxg_sampler_render((size_t)voices, L, voices, sustain ? 1 : 0, d_samples_, len_, l.freq, l.gain, l.par, l.hold, l.pos, l.trig,
                                 l.outhold, l.dst, l.ist, l.mix, nullptr, nullptr), "mxg_sampler_render");
        blk_.resize(L);
        check(mxg_memcpy_d2h(blk_.data(), l.mix, sizeof(double) * L, nullptr), "d2h sampler block");
        end_ = cur_;
        download(end_);
        pos_ = 0;
        launches++;
    }
    // the state at the current sample, cached block dropped: before any control method edits it
    void settle() {
        if (maxigpu::ps::dead()) {
            blk_.clear();
            pos_ = 0;
            return;
        }
        if (!blk_.empty()) {
            if (pos_ == blk_.size()) {
                cur_ = end_;
            } else if (pos_ > 0) {
                render(pos_);
                cur_ = end_;
            }
        }
        blk_.clear();
        pos_ = 0;
        nextLen_ = 1;
    }
    bool valid() const { return voices >= 1 && voices <= kMax; }  // (the reference's arrays hold 32 slots: beyond that it reads out of bounds)

public:
    size_t launches = 0;
    // the reference's public members that its own methods use
    double pitch[32];
    int originalPitch = 67;
    double output = 0;
    double gain = 1;
    int voices = 32;
    int currentVoice = 0;
    bool sustain = true;
    maxiSampler() {  // maxiSynths.cpp:262-283
        for (int i = 0; i < kMax; i++) {
            par_[0 * kMax + i] = mxg_env_coeff_host(0, 0);     // setAttack(0)
            par_[1 * kMax + i] = mxg_env_coeff_host(1, 1);     // setDecay(1)
            par_[2 * kMax + i] = 1.;                            // setSustain(1.)
            par_[3 * kMax + i] = mxg_env_coeff_host(2, 2000);  // setRelease(2000)
            hold_[i] = 1;
            gain_[i] = 0;  // envOutGain: uninitialised in the reference (static storage: 0)
            pitch[i] = 0;
        }
    }
    ~maxiSampler() {
        if (d_samples_) mxg_sample_free(d_samples_);
        if (d_) mxg_free(d_);
    }
    maxiSampler(const maxiSampler &) = delete;
    maxiSampler &operator=(const maxiSampler &) = delete;
    void setNumVoices(int numVoices) {
        settle();
        voices = numVoices;  // maxiSynths.cpp:284-289: any count; the slot arrays hold 32
        if (!valid()) maxigpu::ps::complain("maxiSampler::setNumVoices: 1 .. 32 voices (the reference's slot arrays hold 32) -- other counts play silence");
    }
    void load(string inFile, bool setall = true) {  // maxiSynths.cpp:303-321: samples[i].load(inFile) for every slot
        if (!setall) {  // (the reference loads the file into slot `currentVoice` only)
            maxigpu::ps::complain("maxiSampler::load(file, false): one sample per sampler on this backend (see include/maxiSynths.h) -- not loaded");
            return;
        }
        settle();
        if (d_samples_) mxg_sample_free(d_samples_);
        int32_t hdr[8];
        d_samples_ = mxg_sample_load_wav(inFile.c_str(), 0, &len_, hdr);
        if (!d_samples_) {
            printf("ERROR: Could not load sample.");
            len_ = 0;
            return;
        }
        for (int i = 0; i < kMax; i++) cur_.position[i] = (double)len_;  // maxiSample::read leaves position = size, C:681
    }
    void setSample(vector<double> &sampleData) {  // every samples[i].setSample(sampleData) (H:670-678)
        MAXIGPU_TRY {
        settle();
        if (d_samples_) mxg_sample_free(d_samples_);
        d_samples_ = mxg_sample_upload(sampleData.data(), sampleData.size());
        if (!d_samples_) maxigpu::ps::fatal(std::string("mxg_sample_upload: ") + mxg_last_error());
        len_ = sampleData.size();
        for (int i = 0; i < kMax; i++) cur_.position[i] = (double)len_ - 1;
        }
        MAXIGPU_CATCH(return)
    }
    double play() {  // maxiSynths.cpp:291-311
        if (!d_samples_ || !len_ || !valid() || maxigpu::ps::dead()) return output = 0;  // (a dead device path: silence, nothing touches the device)
        if (pos_ >= blk_.size()) {
            if (!blk_.empty()) cur_ = end_;
            const size_t L = blk_.empty() ? nextLen_ : std::min(2 * blk_.size(), maxigpu::ps::kMaxBlock);
            render(L);
            nextLen_ = L;
        }
        return output = blk_[pos_++];
    }
    void setPitch(double pitchIn, bool setall = false) {  // :323-339
        settle();
        if (setall) for (int i = 0; i < voices; i++) pitch[i] = pitchIn;
        else pitch[currentVoice] = pitchIn;
    }
    void midiNoteOn(double pitchIn, double velocity, bool setall = false) {  // :341-358
        settle();
        if (setall) {
            for (int i = 0; i < voices; i++) pitch[i] = pitchIn;
        } else {
            pitch[currentVoice] = pitchIn;
            gain_[currentVoice] = velocity / 128;
        }
    }
    void midiNoteOff(double pitchIn, double velocity, bool setall = false) {  // :360-372
        (void)velocity; (void)setall;
        settle();
        for (int i = 0; i < voices; i++)
            if (pitch[i] == pitchIn) cur_.trig[i] = 0;
    }
    void setAttack(double attackD, bool setall = true) { set_par(0, mxg_env_coeff_host(0, attackD), setall); }
    void setDecay(double decayD, bool setall = true) { set_par(1, mxg_env_coeff_host(1, decayD), setall); }
    void setSustain(double sustainD, bool setall = true) { set_par(2, sustainD, setall); }
    void setRelease(double releaseD, bool setall = true) { set_par(3, mxg_env_coeff_host(2, releaseD), setall); }
    void setPosition(double positionD, bool setall = true) {  // samples[i].setPosition (C:749-751)
        settle();
        const double p = (positionD < 0.0 ? 0.0 : (positionD > 1.0 ? 1.0 : positionD)) * (double)len_;
        if (setall) for (int i = 0; i < voices; i++) cur_.position[i] = p;
        else cur_.position[currentVoice] = p;
    }
    void trigger() {  // :484-491
        settle();
        cur_.trig[currentVoice] = 1;
        cur_.position[currentVoice] = 0;  // maxiSample::trigger, C:597-600
        currentVoice++;
        currentVoice = currentVoice % voices;
    }

private:
    void set_par(int row, double value, bool setall) {
        settle();
        if (setall) for (int i = 0; i < voices; i++) par_[row * kMax + i] = value;
        else par_[row * kMax + currentVoice] = value;
    }
};

// ---- maxiKick / maxiSnare / maxiHats (src/libs/maxiSynths.h:20-120, maxiSynths.cpp:11-259) --------------------------------------
// DROP-INS for the three drum voices: value types with the reference's public surface, whose play() is ONE launch of the fused drum
// kernel (mxg_drum_render, K21) on a bank of one voice, in the manner of maxiFlanger / maxiDynamics.  What takes effect, read at every
// play(): envelope.attack / decay / sustain / release (setAttack / setDecay / setSustain / setRelease), envelope.holdtime,
// envelope.trigger (trigger() sets it to 1, play() puts a 1 back to 0), the hats' filter.setCutoff / setResonance, and every public
// scalar (pitch, distortion, cutoff, resonance, gain, inverse, useDistortion, useFilter, useLimiter).  Snare and hats draw rand()
// at the call, one draw per play() as maxiOsc::noise does.  Departures, all defined:
//   * cutoff and resonance start at 0.0 where the reference leaves them uninitialised (maxiSnare filters by default): lores clamps
//     them to 10 Hz and 1.
//   * The voice's running state (oscillator phase, envelope state machine, filter state) lives with the drum on the device.  The
//     public sub-objects tone, noise, envelope, distort and filter carry the PARAMETERS; their own running state does not alias the
//     drum's (as maxiFlanger::dl).
//   * The member `output` holds what play() returned (after the gain and the limiter), envOut the envelope's value of the call.
#include "maxiClock.h"

namespace maxigpu {
namespace ps {
template <int KIND>
struct DrumLine {
    // d_blk, doubles unless said.  Uploaded per call, @0..127: trig, pitch, attack, decay, sustain, release, shape, coef [5], gain, (out),
    // holdtime int64, the draw int32.  Read back, @104..223: out, (holdtime, draw), then the state: phase, amplitude, output, int64
    // holdcount + five phase flags, filter state [3].
    static constexpr size_t kBlk = 28 * 8, kArgs = 16 * 8, kState = 16;
    unsigned char *d_blk = nullptr;
    bool init() {
        if (dead()) return false;
        if (d_blk) return true;
        if (!check(mxg_init(-1), "mxg_init")) return false;
        d_blk = static_cast<unsigned char *>(mxg_malloc(kBlk));
        if (!d_blk) {
            check(MXG_ERR_HIP, "mxg_malloc (drum voice)");
            return false;
        }
        return check(mxg_memset(d_blk, 0, kBlk, nullptr), "mxg_memset") && check(mxg_sync(), "mxg_sync");
    }
    void release() {
        if (d_blk) mxg_free(d_blk);
        d_blk = nullptr;
    }
    void copy_from(const DrumLine &o) {
        release();
        if (!o.d_blk || !init()) return;
        check(mxg_memcpy_d2d_async(d_blk, o.d_blk, kBlk, nullptr), "d2d drum state") && check(mxg_stream_sync(nullptr), "mxg_stream_sync");
    }
    // one play(); env_out receives envelope.output after the call
    double run(int flags, bool trig, int32_t draw, double pitch, const double (&par)[4], long holdtime, double shape, const double (&coef)[5],
               double gain, double &env_out) {
        if (!init()) return 0.0;
        double h[kArgs / 8] = {0};
        h[0] = trig ? 1.0 : 0.0;
        h[1] = pitch;
        for (int i = 0; i < 4; i++) h[2 + i] = par[i];
        h[6] = shape;
        for (int i = 0; i < 5; i++) h[7 + i] = coef[i];
        h[12] = gain;
        const int64_t hold = holdtime;
        std::memcpy(&h[14], &hold, 8);
        std::memcpy(&h[15], &draw, 4);
        if (!check(mxg_memcpy_h2d(d_blk, h, kArgs, nullptr), "h2d drum arguments")) return 0.0;
        double *p = reinterpret_cast<double *>(d_blk);
        const int st = mxg_drum_render(KIND, flags, 1, 1, p, 0, KIND == MXG_DRUM_KICK ? nullptr : reinterpret_cast<int32_t *>(p + 15), p + 1, p + 2,
                                       reinterpret_cast<int64_t *>(p + 14), p + 6, p + 7, p + 12, p + kState, p + kState + 1,
                                       reinterpret_cast<int64_t *>(p + kState + 3), p + kState + 9, p + 13, nullptr);
        if (!check(st, "mxg_drum_render")) return 0.0;
        double back[6] = {0};  // out, holdtime, draw, phase, amplitude, envelope.output
        if (!check(mxg_memcpy_d2h(back, d_blk + 13 * 8, sizeof(back), nullptr), "d2h drum output")) return 0.0;
        env_out = back[5];
        return back[0];
    }
};
}  // namespace ps
}  // namespace maxigpu

#define MAXIGPU_DRUM_COMMON(NAME, KIND)                                                                                                  \
    maxigpu::ps::DrumLine<KIND> line_;                                                                                                   \
    void copy_scalars(const NAME &o) {                                                                                                   \
        pitch = o.pitch; output = o.output; outputD = o.outputD; envOut = o.envOut; useDistortion = o.useDistortion;                     \
        useLimiter = o.useLimiter; useFilter = o.useFilter; distortion = o.distortion; inverse = o.inverse; cutoff = o.cutoff;           \
        resonance = o.resonance; gain = o.gain;                                                                                          \
    }                                                                                                                                    \
    int flags_() const {                                                                                                                 \
        return (inverse ? MXG_DRUM_INVERSE : 0) | (useDistortion ? MXG_DRUM_DISTORTION : 0) | (useFilter ? MXG_DRUM_FILTER : 0) |        \
               (useLimiter ? MXG_DRUM_LIMITER : 0);                                                                                      \
    }                                                                                                                                    \
    double play_(int32_t draw, const double (&coef)[5]) {                                                                                \
        const double par[4] = {envelope.attack, envelope.decay, envelope.sustain, envelope.release};                                     \
        double e = 0.0;                                                                                                                  \
        output = line_.run(flags_(), envelope.trigger == 1, draw, pitch, par, envelope.holdtime, distortion, coef, gain, e);             \
        envOut = inverse ? fabs(1 - e) : e;                                                                                              \
        if (envelope.trigger == 1) envelope.trigger = 0;                                                                                 \
        return output;                                                                                                                   \
    }                                                                                                                                    \
    void lores_coef_(double (&coef)[5]) const {                                                                                          \
        double c3[3] = {0, 0, 0};                                                                                                        \
        if (useFilter) maxigpu::ps::check(mxg_filter_coeffs_host(MXG_FLT_LORES, 1, &cutoff, &resonance, c3), "mxg_filter_coeffs_host");  \
        coef[0] = c3[0]; coef[1] = c3[1]; coef[2] = coef[3] = coef[4] = 0.0;                                                             \
    }

class maxiKick {
public:
    maxiKick() {  // maxiSynths.cpp:11-21
        envelope.setAttack(0);
        setPitch(200);
        envelope.setDecay(1);
        envelope.setSustain(1);
        envelope.setRelease(500);
        envelope.holdtime = 1;
        envelope.trigger = 0;
    }
    maxiKick(const maxiKick &o) : kick(o.kick), envelope(o.envelope), distort(o.distort), filter(o.filter) { copy_scalars(o); line_.copy_from(o.line_); }
    maxiKick &operator=(const maxiKick &o) {
        if (this != &o) { kick = o.kick; envelope = o.envelope; distort = o.distort; filter = o.filter; copy_scalars(o); line_.copy_from(o.line_); }
        return *this;
    }
    ~maxiKick() { line_.release(); }
    double play() {  // maxiSynths.cpp:23-73
        double coef[5];
        lores_coef_(coef);
        return play_(0, coef);
    }
    void trigger() { envelope.trigger = 1; }
    void setRelease(double releaseD) { envelope.setRelease(releaseD); }
    // the kick's members are private in the reference: these pairs are its whole parameter surface (the three switch getters
    // return double there too)
    void setPitch(double hz) { pitch = hz; }
    void setDistortion(double shape) { distortion = shape; }
    void setCutoff(double hz) { cutoff = hz; }
    void setResonance(double q) { resonance = q; }
    void setUseDistortion(bool on) { useDistortion = on; }
    void setUseFilter(bool on) { useFilter = on; }
    void setUseLimiter(bool on) { useLimiter = on; }
    double getPitch() const { return pitch; }
    double getDistortion() const { return distortion; }
    double getCutoff() const { return cutoff; }
    double getResonance() const { return resonance; }
    double getUseDistortion() const { return useDistortion ? 1.0 : 0.0; }
    double getUseFilter() const { return useFilter ? 1.0 : 0.0; }
    double getUseLimiter() const { return useLimiter ? 1.0 : 0.0; }

private:
    double pitch = 0;
    double output = 0;
    double outputD = 0;
    double envOut = 0;
    bool useDistortion = false;
    bool useLimiter = false;
    bool useFilter = false;
    double distortion = 0;
    bool inverse = false;
    double cutoff = 0;
    double resonance = 0;
    double gain = 1;
    maxiOsc kick;
    maxiEnv envelope;
    maxiDistortion distort;
    maxiFilter filter;
    MAXIGPU_DRUM_COMMON(maxiKick, MXG_DRUM_KICK)
};

class maxiSnare {
public:
    maxiSnare() {  // maxiSynths.cpp:93-103
        envelope.setAttack(0);
        setPitch(800);
        envelope.setDecay(20);
        envelope.setSustain(0.05);
        envelope.setRelease(300);
        envelope.holdtime = 1;
        envelope.trigger = 0;
    }
    maxiSnare(const maxiSnare &o) : tone(o.tone), noise(o.noise), envelope(o.envelope), distort(o.distort), filter(o.filter) { copy_scalars(o); line_.copy_from(o.line_); }
    maxiSnare &operator=(const maxiSnare &o) {
        if (this != &o) { tone = o.tone; noise = o.noise; envelope = o.envelope; distort = o.distort; filter = o.filter; copy_scalars(o); line_.copy_from(o.line_); }
        return *this;
    }
    ~maxiSnare() { line_.release(); }
    double play() {  // maxiSynths.cpp:105-156
        double coef[5];
        lores_coef_(coef);
        return play_((int32_t)rand(), coef);
    }
    void setPitch(double newPitch) { pitch = newPitch; }
    void setRelease(double releaseD) { envelope.setRelease(releaseD); }
    void trigger() { envelope.trigger = 1; }
    double pitch = 0;
    double output = 0;
    double outputD = 0;
    double envOut = 0;
    bool useDistortion = false;
    bool useLimiter = false;
    bool useFilter = true;
    double distortion = 0;
    bool inverse = false;
    double cutoff = 0;
    double resonance = 0;
    double gain = 1;
    maxiOsc tone;
    maxiOsc noise;
    maxiEnv envelope;
    maxiDistortion distort;
    maxiFilter filter;

private:
    MAXIGPU_DRUM_COMMON(maxiSnare, MXG_DRUM_SNARE)
};

class maxiHats {
public:
    maxiHats() {  // maxiSynths.cpp:176-188
        envelope.setAttack(0);
        setPitch(12000);
        envelope.setDecay(20);
        envelope.setSustain(0.1);
        envelope.setRelease(300);
        envelope.holdtime = 1;
        envelope.trigger = 0;
        filter.setCutoff(8000);
        filter.setResonance(1);
    }
    maxiHats(const maxiHats &o) : tone(o.tone), noise(o.noise), envelope(o.envelope), distort(o.distort), filter(o.filter) { copy_scalars(o); line_.copy_from(o.line_); }
    maxiHats &operator=(const maxiHats &o) {
        if (this != &o) { tone = o.tone; noise = o.noise; envelope = o.envelope; distort = o.distort; filter = o.filter; copy_scalars(o); line_.copy_from(o.line_); }
        return *this;
    }
    ~maxiHats() { line_.release(); }
    double play() {  // maxiSynths.cpp:190-241: the SVF's coefficients are filter's (setCutoff / setResonance); cutoff / resonance are never read
        double coef[5];
        filter.coefficients(coef);
        return play_((int32_t)rand(), coef);
    }
    void setPitch(double newPitch) { pitch = newPitch; }
    void setRelease(double releaseD) { envelope.setRelease(releaseD); }
    void trigger() { envelope.trigger = 1; }
    double pitch = 0;
    double output = 0;
    double outputD = 0;
    double envOut = 0;
    bool useDistortion = false;
    bool useLimiter = false;
    bool useFilter = false;
    double distortion = 0;
    bool inverse = false;
    double cutoff = 0;
    double resonance = 0;
    double gain = 1;
    maxiOsc tone;
    maxiOsc noise;
    maxiEnv envelope;
    maxiDistortion distort;
    maxiSVF filter;

private:
    MAXIGPU_DRUM_COMMON(maxiHats, MXG_DRUM_HATS)
};
#undef MAXIGPU_DRUM_COMMON
