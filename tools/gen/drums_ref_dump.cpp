// tools/gen/drums_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's maxiKick,
// maxiSnare, maxiHats and maxiClock: tools/gen/gen_golden_drums.py compiles it, together with the UNMODIFIED reference sources,
// into a shared library in a temporary directory and drives it to write tests/golden/drums.npz.
//
// One object per run; private members are read and set through -fno-access-control.  The state row after a sample is, in the order
// of mxg_drum_render's state arrays (include/maxigpu.h): oscillator phase | envelope amplitude, output | holdcount, attackphase,
// decayphase, sustainphase, holdphase, releasephase | filter x, y, 0 (kick, snare) or v0z, v1, v2 (hats).
#include <cstdint>
#include <cstdlib>
#include <new>

#include "maximilian.h"
#include "libs/maxiSynths.h"
#include "libs/maxiClock.h"

#define DR_ROWS 12

static void env_rows(const maxiEnv &e, double *r) {
    r[1] = e.amplitude; r[2] = e.output; r[3] = (double)e.holdcount; r[4] = e.attackphase; r[5] = e.decayphase;
    r[6] = e.sustainphase; r[7] = e.holdphase; r[8] = e.releasephase;
}
static void state_row(const maxiKick &d, double *r) { r[0] = d.kick.phase; env_rows(d.envelope, r); r[9] = d.filter.x; r[10] = d.filter.y; r[11] = 0; }
static void state_row(const maxiSnare &d, double *r) { r[0] = d.tone.phase; env_rows(d.envelope, r); r[9] = d.filter.x; r[10] = d.filter.y; r[11] = 0; }
static void state_row(const maxiHats &d, double *r) { r[0] = d.tone.phase; env_rows(d.envelope, r); r[9] = d.filter.v0z; r[10] = d.filter.v1; r[11] = d.filter.v2; }

static void svf_params(maxiKick &, double, double) {}
static void svf_params(maxiSnare &, double, double) {}
static void svf_params(maxiHats &d, double cutoff, double res) { d.filter.setCutoff(cutoff); d.filter.setResonance(res); }

// cfg: 0 pitch (NaN: the constructor's), 1 release ms, 2 decay ms (NaN: the constructor's), 3 useDistortion, 4 distortion, 5 useFilter
// (negative: the class default), 6 cutoff, 7 resonance, 8 useLimiter, 9 gain, 10 inverse, 11 / 12 the hats' filter.setCutoff /
// setResonance (NaN: the constructor's).  trig [N]: trigger() before that play().  out [N]; rows [N + 1][DR_ROWS]: the state in front
// of sample n, rows[N] after the last; envpar [5]: attack, decay, sustain, release, holdtime as the setters left them.
template <class D>
static void run(const double *cfg, size_t N, const uint8_t *trig, double *out, double *rows, double *envpar) {
    srand(1);
    // the reference's constructors leave most members unset; its objects live in static storage: zeroed memory first
    void *mem = calloc(1, sizeof(D));
    D &d = *new (mem) D;
    if (cfg[0] == cfg[0]) d.setPitch(cfg[0]);
    d.setRelease(cfg[1]);
    if (cfg[2] == cfg[2]) d.envelope.setDecay(cfg[2]);
    d.useDistortion = cfg[3] != 0;
    d.distortion = cfg[4];
    if (cfg[5] >= 0) d.useFilter = cfg[5] != 0;
    d.cutoff = cfg[6];
    d.resonance = cfg[7];
    d.useLimiter = cfg[8] != 0;
    d.gain = cfg[9];
    d.inverse = cfg[10] != 0;
    if (cfg[11] == cfg[11]) svf_params(d, cfg[11], cfg[12]);
    envpar[0] = d.envelope.attack; envpar[1] = d.envelope.decay; envpar[2] = d.envelope.sustain; envpar[3] = d.envelope.release;
    envpar[4] = (double)d.envelope.holdtime;
    for (size_t n = 0; n < N; n++) {
        state_row(d, rows + n * DR_ROWS);
        if (trig[n]) d.trigger();
        out[n] = d.play();
    }
    state_row(d, rows + N * DR_ROWS);
    d.~D();
    free(mem);
}

extern "C" {

void dr_set_rate(int sr) { maxiSettings::sampleRate = sr; }

void dr_run(int kind, const double *cfg, size_t N, const uint8_t *trig, double *out, double *rows, double *envpar) {
    if (kind == 0) run<maxiKick>(cfg, N, trig, out, rows, envpar);
    else if (kind == 1) run<maxiSnare>(cfg, N, trig, out, rows, envpar);
    else run<maxiHats>(cfg, N, trig, out, rows, envpar);
}

// the draws rand() hands out after srand(1): one per play() of snare and hats, in call order
void dr_draws(size_t N, int32_t *draws) {
    srand(1);
    for (size_t n = 0; n < N; n++) draws[n] = rand();
}

// maxiClock: setTicksPerBeat, setTempo, optionally setLastCount, then N x ticker()
double dr_clock(int ticks, double tempo, int lastcount, size_t N, uint8_t *tick, int32_t *playhead, int32_t *count, double *phase) {
    void *mem = calloc(1, sizeof(maxiClock));
    maxiClock &c = *new (mem) maxiClock;
    c.setTicksPerBeat(ticks);
    c.setTempo(tempo);
    if (lastcount) c.setLastCount(lastcount);
    for (size_t n = 0; n < N; n++) {
        c.ticker();
        tick[n] = c.tick;
        playhead[n] = c.playHead;
        count[n] = c.currentCount;
        phase[n] = c.timer.phase;
    }
    const double bps = c.bps;
    c.~maxiClock();
    free(mem);
    return bps;
}

}  // extern "C"
