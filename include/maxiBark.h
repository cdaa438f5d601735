// include/maxiBark.h -- drop-in for the reference's src/libs/maxiBark.h: maxiBarkScaleAnalyser<T> / maxiBark, the Bark-scale
// specific, relative and total loudness of one spectrum per call, computed on the device (mxg_bark_batch, K19).  The band sums
// are the reference's bits; pow(sum, 0.23) is the device library's.  Value semantics: a copy is a second
// analyser in the same state.  Before setup() the methods print once and return zeros; once the device path is dead they return
// zeros, as maxiMFCC does.
#pragma once
#include "maximilian.h"

template <class T>
class maxiBarkScaleAnalyser {
public:
    int NUM_BARK_BANDS = MXG_BARK_BANDS;

    maxiBarkScaleAnalyser() { clear(); }
    ~maxiBarkScaleAnalyser() { release(); }
    maxiBarkScaleAnalyser(const maxiBarkScaleAnalyser &o) { clear(); copy_from(o); }
    maxiBarkScaleAnalyser &operator=(const maxiBarkScaleAnalyser &o) { if (this != &o) copy_from(o); return *this; }

    void setup(unsigned int sR, unsigned int bS) {  // L/maxiBark.h:40-62
        MAXIGPU_TRY {
        release();
        sampleRate = sR;
        bufferSize = bS;
        specSize = bS / 2;
        plan_ = mxg_bark_plan_create(sR, bS);
        if (!plan_) maxigpu::ps::fatal(std::string("mxg_bark_plan_create: ") + mxg_last_error());
        d_in_ = static_cast<float *>(mxg_malloc(sizeof(float) * (specSize ? specSize : 1)));
        d_out_ = static_cast<double *>(mxg_malloc(sizeof(double) * (2 * MXG_BARK_BANDS + 1)));
        if (!d_in_ || !d_out_) maxigpu::ps::fatal(std::string("mxg_malloc: ") + mxg_last_error());
        }
        MAXIGPU_CATCH(return)
    }
    double *specificLoudness(float *normalisedSpectrum) {  // :64-75
        run(normalisedSpectrum, 0);
        return specific;
    }
    double *relativeLoudness(float *normalisedSpectrum) {  // :77-97 (it leaves `specific` updated too)
        run(normalisedSpectrum, 1);
        return relative;
    }
    double *totalLoudness(float *normalisedSpectrum) {  // :99-116
        run(normalisedSpectrum, 2);
        return total;
    }

private:
    void clear() {
        for (int i = 0; i < MXG_BARK_BANDS; i++) specific[i] = relative[i] = 0.0;
        total[0] = 0.0;
    }
    void run(const float *spectrum, int which) {
        using maxigpu::ps::check;
        if (!plan_) {
            maxigpu::ps::complain("maxiBark: loudness asked for before setup()");
            return;
        }
        if (maxigpu::ps::dead()) {
            clear();
            return;
        }
        double *d_spec = d_out_, *d_other = d_out_ + MXG_BARK_BANDS;
        check(mxg_memcpy_h2d(d_in_, spectrum, sizeof(float) * specSize, nullptr), "h2d spectrum");
        check(mxg_bark_batch(plan_, d_in_, specSize, 1, nullptr, d_spec, which == 1 ? d_other : nullptr, which == 2 ? d_other : nullptr, nullptr),
              "mxg_bark_batch");
        check(mxg_memcpy_d2h(specific, d_spec, sizeof(double) * MXG_BARK_BANDS, nullptr), "d2h specific");
        if (which == 1) check(mxg_memcpy_d2h(relative, d_other, sizeof(double) * MXG_BARK_BANDS, nullptr), "d2h relative");
        if (which == 2) check(mxg_memcpy_d2h(total, d_other, sizeof(double), nullptr), "d2h total");
    }
    void release() {
        if (plan_) mxg_bark_plan_destroy(plan_);
        if (d_in_) mxg_free(d_in_);
        if (d_out_) mxg_free(d_out_);
        plan_ = nullptr;
        d_in_ = nullptr;
        d_out_ = nullptr;
    }
    void copy_from(const maxiBarkScaleAnalyser &o) {
        if (!o.plan_) release();
        else setup(o.sampleRate, o.bufferSize);
        for (int i = 0; i < MXG_BARK_BANDS; i++) { specific[i] = o.specific[i]; relative[i] = o.relative[i]; }
        total[0] = o.total[0];
    }
    mxg_bark_plan *plan_ = nullptr;
    float *d_in_ = nullptr;
    double *d_out_ = nullptr;
    unsigned int sampleRate = 0, bufferSize = 0, specSize = 0;
    double specific[MXG_BARK_BANDS];
    double relative[MXG_BARK_BANDS];
    double total[1];
};

typedef maxiBarkScaleAnalyser<double> maxiBark;
