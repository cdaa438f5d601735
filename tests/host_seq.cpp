// tests/host_seq.cpp -- host build of mxg_seq.h (tests/test_seq_host.py; the checker of tests/test_gpu_seq.py).
// seq_host_render / seq_host_signal / seq_host_ratio take the arguments of mxg_seq_render / mxg_seq_signal /
// mxg_seq_ratio_host (include/maxigpu.h) without the stream, plus the sample rate, on host arrays in the same layouts, and run
// the step functions a lane of seq.hip's kernels runs, voice after voice.
// With -DSEQ_HOST_MAIN the file is a stand-alone program that plays every path over a few shapes (the sanitizer run).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mxg_seq.h"

using namespace mxg;

static int held(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

extern "C" {

int seq_host_ratio(size_t P, size_t L, const int32_t *len, const double *times, double *norm) {
    for (size_t p = 0; p < P; p++) seq_ratio_bounds(times + p * L, len[p], (int)L, norm + p * L);
    return 0;
}

int seq_host_render(double sr, size_t V, size_t N, const double *freq, double *clk, const double *phase, int phase_pv,
                    const double *norm, const int32_t *len, size_t P, size_t L, const int32_t *pat, int val_mode,
                    const double *values, const int32_t *vlen, size_t PV, size_t LV, const int32_t *vpat, const double *step,
                    const double *hold, double *dst, int64_t *ist, double *trig, double *val, double *gate) {
    int want = 0;
    if (val) want |= val_mode == MXG_SEQ_VAL_STEP ? MXG_SEQ_WANT_STEP : MXG_SEQ_WANT_VALUES;
    if (gate) want |= MXG_SEQ_WANT_GATE;
    for (size_t v = 0; v < V; v++) {
        const int prow = pat ? held(pat[v], 0, (int)P - 1) : 0;
        const int vrow = (val && vpat) ? held(vpat[v], 0, (int)PV - 1) : 0;
        SeqVoiceCfg c;
        c.bounds = norm + (size_t)prow * L;
        c.len = held(len[prow], 1, (int)L);
        c.values = val ? values + (size_t)vrow * LV : norm;
        c.vlen = val ? held(vlen[vrow], 1, (int)LV) : 1;
        c.step = (val && val_mode == MXG_SEQ_VAL_STEP && step) ? step[v] : 1.0;
        c.hold = (gate && hold) ? hold[v] : 0.0;
        c.inv_sr = 1.0 / sr;
        c.want = want;
        SeqRatio r = {dst[v], ist[v] != 0, ist[V + v], ist[2 * V + v]};
        SeqStep st = {{dst[V + v], ist[3 * V + v] != 0}, ist[4 * V + v] != 0, dst[2 * V + v]};
        SeqPulse pu = {{dst[3 * V + v], ist[5 * V + v] != 0}, dst[4 * V + v]};
        double ck = freq ? clk[v] : 0.0;
        const OscPre q = osc_pre<MXG_OSC_PHASOR>(freq ? freq[v] : 0.0, sr, 0.0, 0.0);
        for (size_t n = 0; n < N; n++) {
            const double ph = freq ? seq_clock_tick(ck, q) : (phase_pv ? phase[n * V + v] : phase[n]);
            double t = 0.0, x = 0.0, g = 0.0;
            seq_voice_tick(r, st, pu, c, ph, t, x, g);
            if (trig) trig[n * V + v] = t;
            if (val) val[n * V + v] = x;
            if (gate) gate[n * V + v] = g;
        }
        if (freq) clk[v] = ck;
        dst[v] = r.prevPhase;
        ist[v] = r.first;
        if (want & MXG_SEQ_WANT_VALUES) {
            ist[V + v] = r.counter;
            ist[2 * V + v] = r.lengthOfValues;
        }
        if (want & MXG_SEQ_WANT_STEP) {
            dst[V + v] = st.trig.prev; dst[2 * V + v] = st.index;
            ist[3 * V + v] = st.trig.first; ist[4 * V + v] = st.first;
        }
        if (gate) {
            dst[3 * V + v] = pu.trig.prev; dst[4 * V + v] = pu.hold;
            ist[5 * V + v] = pu.trig.first;
        }
    }
    return 0;
}

int seq_host_signal(int kind, size_t V, size_t N, const double *in, const double *in2, const double *values,
                    const int32_t *vlen, size_t PV, size_t LV, const int32_t *vpat, const double *par, double *dst, int64_t *ist,
                    double *out) {
    const bool tab = kind == MXG_SEQ_STEP || kind == MXG_SEQ_INDEX;
    for (size_t v = 0; v < V; v++) {
        const int vrow = (tab && vpat) ? held(vpat[v], 0, (int)PV - 1) : 0;
        const double *vals = tab ? values + (size_t)vrow * LV : nullptr;
        const int len = tab ? held(vlen[vrow], 1, (int)LV) : 1;
        const double p = par ? par[v] : (kind == MXG_SEQ_STEP ? 1.0 : 0.0);
        double d0 = dst[v], d1 = dst[V + v], d2 = dst[2 * V + v];
        bool f0 = ist[v] != 0, f1 = ist[V + v] != 0;
        for (size_t n = 0; n < N; n++) {
            const double a = in[n * V + v], b = in2 ? in2[n * V + v] : 0.0;
            double y;
            if (kind == MXG_SEQ_ONZX) {
                SeqZx z = {d0, f0};
                y = seq_onzx(z, a);
                d0 = z.prev; f0 = z.first;
            } else if (kind == MXG_SEQ_COUNTER) {
                SeqCounter k = {d0, {d1, f0}, {d2, f1}};
                y = seq_counter(k, a, b);
                d0 = k.value; d1 = k.inc.prev; f0 = k.inc.first; d2 = k.rst.prev; f1 = k.rst.first;
            } else if (kind == MXG_SEQ_STEP) {
                SeqStep s = {{d0, f0}, f1, d1};
                y = seq_step_pull(s, a, vals, len, p);
                d0 = s.trig.prev; f0 = s.trig.first; f1 = s.first; d1 = s.index;
            } else if (kind == MXG_SEQ_INDEX) {
                SeqIndex x = {{d0, f0}, d1};
                y = seq_index_pull(x, a, b, vals, len);
                d0 = x.trig.prev; f0 = x.trig.first; d1 = x.value;
            } else {
                SeqPulse q = {{d0, f0}, d1};
                y = seq_pulse(q, a, p);
                d0 = q.trig.prev; f0 = q.trig.first; d1 = q.hold;
            }
            out[n * V + v] = y;
        }
        dst[v] = d0; dst[V + v] = d1; dst[2 * V + v] = d2;
        ist[v] = f0; ist[V + v] = f1;
    }
    return 0;
}

// maxiOsc::saw with a frequency per sample (mxg_osc_render, fps = 1): the oscillator leg of the chained test
int seq_host_saw(double sr, size_t V, size_t N, const double *freq, double *phase, double *out) {
    for (size_t v = 0; v < V; v++) {
        double ph = phase[v], hd = 0.0;
        for (size_t n = 0; n < N; n++) {
            const OscPre q = osc_pre<MXG_OSC_SAW>(freq[n * V + v], sr, 0.0, 0.0);
            out[n * V + v] = osc_tick<MXG_OSC_SAW>(ph, hd, q, nullptr, nullptr);
        }
        phase[v] = ph;
    }
    return 0;
}

}  // extern "C"

#ifdef SEQ_HOST_MAIN
// Every path once, over shapes that cross the chunk edges, with steps that leave the table (the held index) and a zero sum.
int main() {
    const size_t P = 4, L = 7, PV = 3, LV = 10;
    const int32_t len[P] = {3, 1, 7, 2}, vlen[PV] = {1, 6, 10};
    const double times[P * L] = {3, 3, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 4, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> norm(P * L), values(PV * LV);
    for (size_t i = 0; i < values.size(); i++) values[i] = 100.0 + (double)i;
    seq_host_ratio(P, L, len, times, norm.data());
    unsigned long long acc = 0;
    for (size_t V : {1, 2, 5}) {
        for (size_t N : {1, 7, 8, 9, 600}) {
            std::vector<int32_t> pat(V), vpat(V);
            std::vector<double> freq(V), step(V), hold(V), clk(V, 0.0), dst(5 * V, 0.0), sd(3 * V, 0.0);
            std::vector<int64_t> ist(6 * V, 0), si(2 * V, 1);
            const double steps[6] = {1, 2, -1, 0.5, 13, -25};
            for (size_t v = 0; v < V; v++) {
                pat[v] = (int)(v % P); vpat[v] = (int)(v % PV);
                freq[v] = 700.0 + 300.0 * v; step[v] = steps[v % 6]; hold[v] = 2.5 * v;
                dst[V + v] = dst[3 * V + v] = 1.0;
                ist[v] = ist[3 * V + v] = ist[4 * V + v] = ist[5 * V + v] = 1;
                sd[v] = 1.0;
            }
            std::vector<double> t(N * V), x(N * V), g(N * V), o(N * V);
            for (int mode = 0; mode < 2; mode++) {
                seq_host_render(44100.0, V, N, freq.data(), clk.data(), nullptr, 0, norm.data(), len, P, L, pat.data(), mode,
                                values.data(), vlen, PV, LV, vpat.data(), step.data(), hold.data(), dst.data(), ist.data(), t.data(),
                                x.data(), g.data());
                seq_host_render(44100.0, V, N, nullptr, nullptr, x.data(), 1, norm.data(), len, P, L, nullptr, mode, values.data(),
                                vlen, PV, LV, nullptr, nullptr, nullptr, dst.data(), ist.data(), nullptr, x.data(), nullptr);
            }
            for (int kind = 0; kind <= MXG_SEQ_ZXTOPULSE; kind++) {
                seq_host_signal(kind, V, N, t.data(), g.data(), values.data(), vlen, PV, LV, vpat.data(), step.data(), sd.data(),
                                si.data(), o.data());
                for (double y : o) acc += (unsigned long long)(y < 0 ? -y : y);
            }
        }
    }
    printf("host_seq: ok (%llu)\n", acc);
    return 0;
}
#endif
