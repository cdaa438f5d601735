// tests/patches/fuzz_patch.cpp -- a SEEDED RANDOM patch in the reference's plugin form: setup() draws a graph of 8-24 unit generators
// (maxiOsc / maxiFilter / maxiEnv / maxiDelayline / maxiSample / maxiSVF / maxiBiquad / maxiDCBlocker / maxiEnvGen, and in one profile
// maxiFlanger / maxiChorus) whose arguments are literals, forms the per-sample engine of include/maximilian.h can derive from other
// objects' outputs (x, x*a, x+b, x*a+b, (x+b)*a, x1+x2, (x1+x2)*a, x1*x2, ((x+b)*a)+c), the same over LAST frame's outputs (feedback), or
// forms it cannot fit; play() then draws rare events per frame (a changed literal, another method, a setter, a public state member read
// and written, copies, a growing vector, an object destroyed and constructed again, calls skipped or doubled, delay sizes changed on the
// block edges).  TEST INFRASTRUCTURE: compiled once against the reference (oracle/Makefile _ref/example_fz -> tests/golden/dropin_fuzz.npz)
// and once against include/maximilian.h (host/Makefile dropin_fz); tests/test_gpu_dropin_fuzz.py compares the streams bit for bit.
//   MXG_FUZZ_SEED, MXG_FUZZ_PROFILE (0-3), MXG_FUZZ_FRAMES (the run's length: profile 3 needs it), MXG_FUZZ_MAXOBJ (cap, minimising),
//   MXG_FUZZ_LOG=1 (one line per event on stdout: frame kind object).  Counts of events and calls go to stderr at exit ("FUZZ ...").
// Rules of the file: all randomness from the xorshift below (rand() belongs to maxiOsc::noise / maxiChorus); every number computed here
// comes from IEEE + - * / on doubles and integer arithmetic (no libm), so both builds round it identically; every object is a heap copy
// of a never-called object with static storage (the reference leaves members uninitialised: static-storage zeros are the defined start);
// no call reaches what the reference leaves undefined (table frequencies inside [0, sr/2], delay sizes inside the ring, play heads kept
// off the last two samples of a buffer, phase families kept apart when a method changes).
#include "maximilian.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    uint32_t u(uint32_t n) { return (uint32_t)((next() >> 33) % n); }
    bool chance(uint32_t num, uint32_t den) { return u(den) < num; }
    double frac() { return (double)(next() >> 11 & 0xFFFFF) / 1048583.0; }  // [0, 1), no short decimal
};
Rng G, E;  // the graph's draws (setup), the events' draws (play)

enum Cls { OSC, FLT, ENV, DLY, SMP, SVF, BIQ, DCB, EGN, FLG, CHO, NCLS };
const char *kClsName[NCLS] = {"osc", "flt", "env", "dly", "smp", "svf", "biq", "dcb", "egn", "flg", "cho"};
enum Dom { D_IN, D_FREQ, D_LFO, D_CUT, D_UNIT, D_RES, D_BPRES, D_LO, D_HI, D_SIZE, D_FB, D_SPEED, D_PF, D_R, D_DEPTH, D_FXDELAY, D_TABF, NDOM };
// a domain, and three (s, k, c) triples of short decimals with c = s * k: x * s + c and (x + k) * s stay inside it for x in [-1, 1]
struct DomSpec { double lo, hi, s[3], k[3], c[3]; };
const DomSpec kDom[NDOM] = {
    {-4, 4, {0.5, 0.25, 0.8}, {0.2, 0.4, 0.25}, {0.1, 0.1, 0.2}},
    {20, 5000, {100, 50, 200}, {4, 6, 5}, {400, 300, 1000}},
    {0.1, 40, {2, 0.5, 1}, {5, 4, 3}, {10, 2, 3}},
    {50, 8000, {300, 100, 500}, {5, 6, 4}, {1500, 600, 2000}},
    {0.02, 0.98, {0.1, 0.05, 0.1}, {5, 6, 4}, {0.5, 0.3, 0.4}},
    {1, 8, {0.5, 0.25, 0.5}, {6, 8, 4}, {3, 2, 2}},
    {0.05, 0.4, {0.02, 0.05, 0.02}, {10, 5, 5}, {0.2, 0.25, 0.1}},
    {0, 0.4, {0.05, 0.02, 0.05}, {4, 5, 2}, {0.2, 0.1, 0.1}},
    {0.6, 1, {0.05, 0.02, 0.02}, {16, 40, 45}, {0.8, 0.8, 0.9}},
    {1, 3000, {100, 200, 10}, {5, 6, 4}, {500, 1200, 40}},
    {0, 0.95, {0.1, 0.1, 0.05}, {5, 7, 6}, {0.5, 0.7, 0.3}},
    {0.25, 2, {0.2, 0.1, 0.25}, {5, 7, 6}, {1, 0.7, 1.5}},
    {0.5, 20, {1, 0.5, 2}, {4, 4, 5}, {4, 2, 10}},
    {0.9, 0.999, {0.01, 0.005, 0.01}, {95, 198, 97}, {0.95, 0.99, 0.97}},
    {0.05, 0.3, {0.02, 0.05, 0.02}, {10, 3, 5}, {0.2, 0.15, 0.1}},
    {1, 500, {20, 50, 5}, {5, 6, 6}, {100, 300, 30}},
    {1, 20000, {100, 500, 20}, {4, 6, 5}, {400, 3000, 100}},   // wavetable oscillators: inside [0, sr/2]
};
double into(double v, int d) {  // the guard that brings an argument into its domain (NaN -> lo)
    if (!(v >= kDom[d].lo)) v = kDom[d].lo;
    if (v > kDom[d].hi) v = kDom[d].hi;
    return v;
}

// kinds of an argument
enum { A_LIT, A_ODD, A_CUR, A_PREV, A_UNFIT };
struct Arg {
    int kind = A_LIT, form = 4, dom = D_IN, s1 = 0, s2 = 0, s3 = 0;
    double lit = 0, a = 1, b = 0, c = 0;
    double once = 0;
    bool hasOnce = false;
};

const int kMaxArgs = 5;
struct Obj {
    int cls = OSC, method = 0, family = 0;
    Arg arg[kMaxArgs];
    double out = 0, prev = 0, w = 0.1;
    int skip = 0;
    bool twice = false;
    // envelope / envelope generator gates
    int trigMode = 0, trigSrc = 0, period = 3000, gateLen = 800;
    double thr = 0;
    double att = 0.01, dec = 0.9995, sus = 0.4, rel = 0.9997;  // parameters re-applied when the object is constructed again
    long hold = 100;
    double p1 = 1000, p2 = 1, p3 = 0;
    int itype = 0;
    bool loop = false;
    // sample
    int data = 0;
    double posBound = 0;
    double start = 10, end = 3000;
    // delay line
    long sinceChange = 0;
    int position = 0;
    maxiOsc *osc = nullptr;
    maxiFilter *flt = nullptr;
    maxiEnv *env = nullptr;
    maxiDelayline *dly = nullptr;
    maxiSample *smp = nullptr;
    maxiSVF *svf = nullptr;
    maxiBiquad *biq = nullptr;
    maxiDCBlocker *dcb = nullptr;
    maxiEnvGen *egn = nullptr;
    maxiFlanger *flg = nullptr;
    maxiChorus *cho = nullptr;
};

// never called: what a new object is a copy of
maxiOsc pristineOsc;
maxiFilter pristineFlt;
maxiEnv pristineEnv;
maxiDelayline pristineDly;
maxiSample pristineSmp;
maxiSVF pristineSvf;
maxiBiquad pristineBiq;
maxiDCBlocker pristineDcb;
maxiEnvGen pristineEgn;
maxiFlanger pristineFlg;
maxiChorus pristineCho;

std::vector<Obj> objs;
std::vector<double> sampleData[2];
std::vector<maxiOsc> vOsc;     // vectors that grow (a reallocation copies every element) and shrink
std::vector<maxiEnv> vEnv;
std::vector<maxiFilter> vFlt;
long frame = 0, totalFrames = 6000;
int profile = 0;
bool logEvents = false;
unsigned memberOp = 0;
double extra = 0;  // what events add to channel 0 of this frame

// ---- counts (stderr at exit) ----
long evCount[10];
enum { M_PHASOR, M_SAW, M_TRIANGLE, M_SQUARE, M_PULSE, M_IMPULSE, M_PHASORBETWEEN, M_SAWN, M_SINEBUF, M_SINEBUF4, M_NOISE, M_PHASERESET,
       M_LORES, M_HIRES, M_BANDPASS, M_LOPASS, M_HIPASS, M_SETCUTOFF, M_SETRESONANCE,
       M_ADSR, M_ADSR2, M_AR, M_SETATTACK, M_SETDECAY, M_SETSUSTAIN, M_SETRELEASE, M_ENVMEMBER,
       M_DL, M_DLFROMPOSITION,
       M_PLAY, M_PLAYONCE, M_PLAYATSPEED, M_PLAYATSPEEDBETWEENPOINTS, M_PLAY4, M_TRIGGER, M_SETPOSITION,
       M_SVF, M_SVFSET, M_BIQUAD, M_BIQUADSET, M_DCBLOCKER, M_ENVGEN, M_ENVGENSETUP, M_FLANGE, M_CHORUS,
       M_COPYASSIGN, M_COPYTEMP, M_VECGROW, M_VECSHRINK, M_RECONSTRUCT, M_SKIP, M_TWICE, M_GROUPS, M_NCOUNT };
const char *kCountName[M_NCOUNT] = {
    "phasor", "saw", "triangle", "square", "pulse", "impulse", "phasorBetween", "sawn", "sinebuf", "sinebuf4", "noise", "phaseReset",
    "lores", "hires", "bandpass", "lopass", "hipass", "setCutoff", "setResonance",
    "adsr", "adsr2", "ar", "setAttack", "setDecay", "setSustain", "setRelease", "envMember",
    "dl", "dlFromPosition",
    "play", "playOnce", "playAtSpeed", "playAtSpeedBetweenPoints", "play4", "trigger", "setPosition",
    "svf", "svfSet", "biquad", "biquadSet", "dcblocker", "envgen", "envgenSetup", "flange", "chorus",
    "copyAssign", "copyTemp", "vecGrow", "vecShrink", "reconstruct", "skip", "twice", "groups"};
long mCount[M_NCOUNT];
long opCount[9];  // the StateMember operators: = T, = member, +=, -=, *=, /=, ++, --, read
void report() {
    std::fprintf(stderr, "FUZZ profile=%d frames=%ld objects=%d", profile, frame, (int)objs.size());
    for (int k = 1; k <= 9; k++) std::fprintf(stderr, " ev%d=%ld", k, evCount[k]);
    for (int k = 0; k < M_NCOUNT; k++) std::fprintf(stderr, " %s=%ld", kCountName[k], mCount[k]);
    for (int k = 0; k < 9; k++) std::fprintf(stderr, " op%d=%ld", k, opCount[k]);
    std::fprintf(stderr, "\n");
}
void logEvent(int kind, int obj) {
    evCount[kind]++;
    if (logEvents) std::printf("%ld %d %d %s\n", frame, kind, obj, obj >= 0 ? kClsName[objs[(size_t)obj].cls] : "-");
}

// ---- arguments ----
double shortLit(Rng &r, int d) {  // a short decimal inside the domain
    const int t = (int)r.u(3);
    const DomSpec &D = kDom[d];
    const uint32_t w = r.u(3);
    double v = w == 0 ? D.c[t] : (w == 1 ? D.c[t] + D.s[t] : D.c[t] - D.s[t]);
    return into(v, d);
}
double oddLit(Rng &r, int d) {  // no short decimal
    const DomSpec &D = kDom[d];
    double v = D.lo + (D.hi - D.lo) * (0.1 + 0.8 * r.frac());
    if (d == D_FREQ || d == D_CUT || d == D_TABF || d == D_SIZE) v = D.lo + (D.hi - D.lo) * 0.3 * r.frac() + 1.0 / 3.0;
    return into(v, d);
}
Arg drawArg(Rng &r, int d, int self, bool signal) {
    Arg A;
    A.dom = d;
    const uint32_t p = r.u(100);
    if (signal) A.kind = p < 10 ? A_LIT : (p < 15 ? A_ODD : (p < 55 ? A_CUR : (p < 80 ? A_PREV : A_UNFIT)));
    else A.kind = p < 40 ? A_LIT : (p < 55 ? A_ODD : (p < 72 ? A_CUR : (p < 87 ? A_PREV : A_UNFIT)));
    if (self == 0 && A.kind == A_CUR) A.kind = A_PREV;  // nothing earlier in this frame
    const int n = self < 0 ? 1 : (A.kind == A_CUR ? self : (int)objs.size() + 1);  // PREV / UNFIT: any object drawn so far, itself included
    A.s1 = (int)r.u((uint32_t)n);
    A.s2 = (int)r.u((uint32_t)n);
    A.s3 = (int)r.u((uint32_t)n);
    if (A.kind == A_CUR && self >= 2 && r.chance(1, 2)) {  // the two objects called just before this one
        A.s1 = self - 1;
        A.s2 = self - 2;
    }
    const int t = (int)r.u(3);
    const DomSpec &D = kDom[d];
    A.lit = A.kind == A_ODD ? oddLit(r, d) : shortLit(r, d);
    if (A.kind == A_UNFIT) {
        A.form = 10 + (int)r.u(3);
        A.a = D.s[t];
        A.b = D.c[t];
    } else if (d == D_IN) {
        A.form = 1 + (int)r.u(9);
        static const double as[4] = {0.5, 0.25, 0.8, 1.5}, bs[4] = {0.1, -0.2, 0.05, 0.3}, cs[3] = {0.01, -0.3, 0.125};
        A.a = as[r.u(4)];
        A.b = bs[r.u(4)];
        A.c = cs[r.u(3)];
    } else {  // a parameter with a domain: the forms that have an offset
        static const int fs[4] = {3, 4, 5, 9};
        static const double inner[3] = {1, 2, -1};
        A.form = fs[r.u(4)];
        A.a = D.s[t];
        A.b = A.form == 5 ? D.k[t] : (A.form == 9 ? inner[r.u(3)] : D.c[t]);
        A.c = D.c[t];
    }
    return A;
}
double clamp4(double v) {
    if (!(v >= -4.0)) v = -4.0;
    if (v > 4.0) v = 4.0;
    return v;
}
double source(const Arg &A, int s) {
    const Obj &o = objs[(size_t)s < objs.size() ? (size_t)s : 0];
    return A.kind == A_CUR ? o.out : clamp4(o.prev);  // feedback edges pass through the clamp
}
double evalArg(Arg &A) {
    if (A.hasOnce) {
        A.hasOnce = false;
        return into(A.once, A.dom);
    }
    if (A.kind == A_LIT || A.kind == A_ODD) return A.lit;
    const double x1 = source(A, A.s1), x2 = source(A, A.s2), x3 = source(A, A.s3);
    double t = 0;
    switch (A.form) {  // statement by statement: one rounding each
        case 1: t = x1; break;
        case 2: t = x1 * A.a; break;
        case 3: t = x1 + A.b; break;
        case 4: t = x1 * A.a; t = t + A.b; break;
        case 5: t = x1 + A.b; t = t * A.a; break;
        case 6: t = x1 + x2; break;
        case 7: t = x1 + x2; t = t * A.a; break;
        case 8: t = x1 * x2; break;
        case 9: t = x1 + A.b; t = t * A.a; t = t + A.c; break;
        case 10: t = x1 * x2; t = t * x3; t = t * A.a; t = t + A.b; break;            // a product of three outputs
        case 11: t = x2 * x2; t = t + 1.5; t = x1 / t; t = t * A.a; t = t + A.b; break;  // a quotient
        default: t = x1 > 0 ? A.b + A.a : A.b - A.a; break;                          // a comparison
    }
    return into(t, A.dom);
}

// ---- objects ----
void applyParams(Obj &o) {  // the setters an object gets after construction
    switch (o.cls) {
        case ENV:
            o.env->attack = o.att; o.env->decay = o.dec; o.env->sustain = o.sus; o.env->release = o.rel;
            o.env->holdtime = o.hold;
            o.env->trigger = 0;
            break;
        case FLT: o.flt->setCutoff(o.p1); o.flt->setResonance(o.p2); break;
        case SMP:
            if (o.data == 0) o.smp->setSample(sampleData[0]); else o.smp->setSampleAndRate(sampleData[1], 22050);
            o.smp->trigger();  // (setSample leaves the head on the last sample)
            o.posBound = 0;
            break;
        case SVF: o.svf->setCutoff(o.p1); o.svf->setResonance(o.p2); mCount[M_SVFSET]++; break;
        case BIQ: o.biq->set((maxiBiquad::filterTypes)o.itype, o.p1, o.p2, o.p3); mCount[M_BIQUADSET]++; break;
        case EGN:
            if (o.loop) o.egn->setup({o.sus, 1, o.sus}, {o.p1, o.p2}, {1, 1}, true);
            else o.egn->setupADSR(o.p1, o.p2, o.sus, o.p3);
            mCount[M_ENVGENSETUP]++;
            break;
        default: break;
    }
}
void construct(Obj &o) {
    switch (o.cls) {
        case OSC: o.osc = new maxiOsc(pristineOsc); break;
        case FLT: o.flt = new maxiFilter(pristineFlt); break;
        case ENV: o.env = new maxiEnv(pristineEnv); break;
        case DLY: o.dly = new maxiDelayline(pristineDly); break;
        case SMP: o.smp = new maxiSample(pristineSmp); break;
        case SVF: o.svf = new maxiSVF(pristineSvf); break;
        case BIQ: o.biq = new maxiBiquad(pristineBiq); break;
        case DCB: o.dcb = new maxiDCBlocker(pristineDcb); break;
        case EGN: o.egn = new maxiEnvGen(pristineEgn); break;
        case FLG: o.flg = new maxiFlanger(pristineFlg); break;
        case CHO: o.cho = new maxiChorus(pristineCho); break;
    }
    applyParams(o);
}
void destroy(Obj &o) {
    delete o.osc; delete o.flt; delete o.env; delete o.dly; delete o.smp; delete o.svf; delete o.biq; delete o.dcb; delete o.egn;
    delete o.flg; delete o.cho;
    o.osc = nullptr; o.flt = nullptr; o.env = nullptr; o.dly = nullptr; o.smp = nullptr; o.svf = nullptr; o.biq = nullptr;
    o.dcb = nullptr; o.egn = nullptr; o.flg = nullptr; o.cho = nullptr;
}
int gateOf(const Obj &o) {
    if (o.trigMode == 0) return (frame % o.period) < o.gateLen ? 1 : 0;
    return clamp4(objs[(size_t)o.trigSrc].prev) > o.thr ? 1 : 0;  // another object's output crossing a threshold
}
size_t dataLen(const Obj &o) { return sampleData[o.data].size(); }

// one call of the object's current method on `o` -- or, for the temporaries of event 5, on copies passed in `t`
double callOn(Obj &o, const double *v, Obj &t) {
    switch (o.cls) {
        case OSC:
            switch (o.method) {
                case 0: mCount[M_PHASOR]++; return t.osc->phasor(v[0]);
                case 1: mCount[M_SAW]++; return t.osc->saw(v[0]);
                case 2: mCount[M_TRIANGLE]++; return t.osc->triangle(v[0]);
                case 3: mCount[M_SQUARE]++; return t.osc->square(v[0]);
                case 4: mCount[M_PULSE]++; return t.osc->pulse(v[0], v[1]);
                case 5: mCount[M_IMPULSE]++; return t.osc->impulse(v[0]);
                case 6: mCount[M_PHASORBETWEEN]++; return t.osc->phasorBetween(v[0], v[2], v[3]);
                case 7: mCount[M_SAWN]++; return t.osc->sawn(v[0]);
                case 8: mCount[M_SINEBUF]++; return t.osc->sinebuf(v[0]);
                case 9: mCount[M_SINEBUF4]++; return t.osc->sinebuf4(v[0]);
                default: mCount[M_NOISE]++; return t.osc->noise();
            }
        case FLT:
            switch (o.method) {
                case 0: mCount[M_LORES]++; return t.flt->lores(v[0], v[1], v[2]);
                case 1: mCount[M_HIRES]++; return t.flt->hires(v[0], v[1], v[2]);
                case 2: mCount[M_BANDPASS]++; return t.flt->bandpass(v[0], v[1], v[3]);
                case 3: mCount[M_LOPASS]++; return t.flt->lopass(v[0], v[4]);
                default: mCount[M_HIPASS]++; return t.flt->hipass(v[0], v[4]);
            }
        case ENV: {
            const int g = gateOf(o);
            maxiEnv &e = *t.env;
            switch (o.method) {
                case 0: mCount[M_ADSR]++; return e.adsr(v[0], e.attack, e.decay, e.sustain, e.release, e.holdtime, g);
                case 1: mCount[M_ADSR2]++; e.trigger = g; return e.adsr(v[0], e.trigger);
                default: mCount[M_AR]++; return e.ar(v[0], e.attack, e.release, e.holdtime, g);
            }
        }
        case DLY: {
            const int size = (int)v[1];
            if (o.method == 0) { mCount[M_DL]++; return t.dly->dl(v[0], size, v[2]); }
            mCount[M_DLFROMPOSITION]++;
            return t.dly->dlFromPosition(v[0], size, v[2], o.position % size);
        }
        case SMP:
            switch (o.method) {
                case 0: mCount[M_PLAY]++; return t.smp->play();
                case 1: mCount[M_PLAYONCE]++; return t.smp->playOnce();
                case 2:  // the head advances by at most `speed` a call: back to 0 before it can reach the buffer's last two samples
                    if (&t == &o) {
                        if (o.posBound + v[1] > (double)dataLen(o) - 4.0) {
                            o.smp->trigger();
                            o.posBound = 0;
                        }
                        o.posBound = o.posBound + v[1];
                    }
                    mCount[M_PLAYATSPEED]++;
                    return t.smp->playAtSpeed(v[1]);
                case 3: mCount[M_PLAYATSPEEDBETWEENPOINTS]++; return t.smp->playAtSpeedBetweenPoints(v[2], o.start, o.end);
                default: mCount[M_PLAY4]++; return t.smp->play4(v[2], o.start, o.end);
            }
        case SVF: mCount[M_SVF]++; return t.svf->play(v[0], v[1], v[2], v[3], v[4]);
        case BIQ: mCount[M_BIQUAD]++; return t.biq->play(v[0]);
        case DCB: mCount[M_DCBLOCKER]++; return t.dcb->play(v[0], v[1]);
        case EGN: mCount[M_ENVGEN]++; return t.egn->play(o.loop ? 1.0 : (gateOf(o) ? 1.0 : -1.0));
        case FLG: mCount[M_FLANGE]++; return t.flg->flange(v[0], (unsigned int)v[1], v[2], v[3], v[4]);
        default: mCount[M_CHORUS]++; return t.cho->chorus(v[0], (unsigned int)v[1], v[2], v[3], v[4]);
    }
}

int nArgs(int cls) {
    static const int n[NCLS] = {4, 5, 1, 3, 3, 5, 1, 2, 0, 5, 5};
    return n[cls];
}
void drawArgs(Obj &o, int self) {
    static const int doms[NCLS][kMaxArgs] = {
        {D_FREQ, D_UNIT, D_LO, D_HI, D_IN},            // osc: frequency, duty, start phase, end phase
        {D_IN, D_CUT, D_RES, D_BPRES, D_UNIT},         // filter: input, cutoff, resonance, bandpass resonance, one-pole cutoff
        {D_IN, D_IN, D_IN, D_IN, D_IN},                // env: input
        {D_IN, D_SIZE, D_FB, D_IN, D_IN},              // delay: input, size, feedback
        {D_IN, D_SPEED, D_PF, D_IN, D_IN},             // sample: -, speed, frequency
        {D_IN, D_UNIT, D_UNIT, D_UNIT, D_UNIT},        // svf: input, four mixes
        {D_IN, D_IN, D_IN, D_IN, D_IN},                // biquad: input
        {D_IN, D_R, D_IN, D_IN, D_IN},                 // dc blocker: input, R
        {D_IN, D_IN, D_IN, D_IN, D_IN},
        {D_IN, D_FXDELAY, D_FB, D_LFO, D_DEPTH},       // flanger / chorus: input, delay, feedback, speed, depth
        {D_IN, D_FXDELAY, D_FB, D_LFO, D_DEPTH},
    };
    for (int k = 0; k < nArgs(o.cls); k++) {
        int d = doms[o.cls][k];
        if (o.cls == OSC && k == 0) d = o.family == 1 ? D_TABF : (G.chance(1, 3) ? D_LFO : D_FREQ);
        o.arg[k] = drawArg(G, d, self, d == D_IN);
        if (o.cls == ENV && G.chance(1, 2)) { o.arg[k].kind = A_LIT; o.arg[k].lit = 1.0; }
        if (o.cls == DLY && k == 1 && o.arg[k].kind != A_LIT && G.chance(2, 3)) o.arg[k].kind = A_LIT;  // sizes mostly move by event 9
    }
}
void drawMethod(Obj &o, Rng &r) {
    switch (o.cls) {
        case OSC:
            if (o.family == 0) o.method = (int)r.u(8);
            else if (o.family == 1) o.method = 8 + (int)r.u(2);
            else o.method = 10;
            break;
        case FLT: o.method = (int)r.u(5); break;
        case ENV: o.method = (int)r.u(3); break;
        case DLY: o.method = (int)r.u(2); break;
        case SMP: o.method = (int)r.u(5); break;
        default: o.method = 0; break;
    }
}
void drawParams(Obj &o, Rng &r) {
    static const double atts[4] = {0.001, 0.01, 0.0005, 0.05}, decs[4] = {0.9995, 0.999, 0.99, 0.9999};
    o.att = atts[r.u(4)];
    o.dec = decs[r.u(4)];
    o.rel = decs[r.u(4)];
    o.sus = shortLit(r, D_UNIT);
    o.hold = 1 + (long)r.u(500);
    switch (o.cls) {
        case FLT: o.p1 = shortLit(r, D_CUT); o.p2 = shortLit(r, D_RES); break;
        case SVF: o.p1 = r.chance(1, 2) ? shortLit(r, D_CUT) : oddLit(r, D_CUT); o.p2 = 0.5 + 0.5 * (double)r.u(9); break;
        case BIQ: o.itype = (int)r.u(7); o.p1 = shortLit(r, D_CUT); o.p2 = 0.5 + 0.25 * (double)r.u(12); o.p3 = (double)r.u(13) - 6.0; break;
        case EGN:
            o.loop = r.chance(1, 2);
            o.p1 = 5 + (double)r.u(60);
            o.p2 = 20 + (double)r.u(100);
            o.p3 = 30 + (double)r.u(200);
            if (o.loop) o.sus = 0.1 * (double)(1 + r.u(5));
            break;
        default: break;
    }
}

Obj drawObject(int cls, int self) {
    Obj o;
    o.cls = cls;
    if (cls == OSC) {
        const uint32_t f = G.u(10);
        o.family = f < 6 ? 0 : (f < 9 ? 1 : 2);
    }
    drawMethod(o, G);
    drawArgs(o, self);
    drawParams(o, G);
    static const double ws[6] = {0.1, 0.05, 0.2, -0.1, 0.15, -0.05};
    o.w = ws[G.u(6)];
    o.trigMode = self > 0 && G.chance(1, 3) ? 1 : 0;
    o.trigSrc = self > 0 ? (int)G.u((uint32_t)self) : 0;
    o.thr = 0.1 * (double)G.u(5);
    o.period = 500 + (int)G.u(3000);
    o.gateLen = 50 + (int)G.u((uint32_t)o.period / 2);
    o.data = (int)G.u(2);
    o.start = 1 + (double)G.u(1000);
    o.end = 2000 + (double)G.u(900);
    o.position = (int)G.u(3000);
    return o;
}

int pickClass() {
    static const int w[4][NCLS] = {
        {6, 4, 3, 2, 3, 1, 1, 1, 1, 0, 0},
        {6, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0},
        {3, 1, 0, 5, 5, 0, 0, 0, 0, 1, 1},
        {6, 4, 3, 2, 3, 1, 1, 1, 1, 0, 0},
    };
    int total = 0;
    for (int c = 0; c < NCLS; c++) total += w[profile][c];
    int p = (int)G.u((uint32_t)total);
    for (int c = 0; c < NCLS; c++) {
        p -= w[profile][c];
        if (p < 0) return c;
    }
    return OSC;
}

bool eventsOn() { return profile != 3 || frame < 1000 || frame >= totalFrames - 500; }

// another live object of the same class, or -1
int peer(int i) {
    std::vector<int> c;
    for (size_t j = 0; j < objs.size(); j++)
        if ((int)j != i && objs[j].cls == objs[(size_t)i].cls) c.push_back((int)j);
    return c.empty() ? -1 : c[E.u((uint32_t)c.size())];
}

void changeLiteral(Obj &o, bool once) {  // event 1
    const int n = nArgs(o.cls);
    if (n == 0) return;
    Arg &A = o.arg[E.u((uint32_t)n)];
    const double v = E.chance(1, 2) ? shortLit(E, A.dom) : oddLit(E, A.dom);
    if (once) {
        A.once = v;
        A.hasOnce = true;
    } else if (A.kind == A_LIT || A.kind == A_ODD) {
        A.lit = v;
    } else {  // the literal inside the expression
        const int t = (int)E.u(3);
        if (A.form == 5) { A.a = kDom[A.dom].s[t]; A.b = kDom[A.dom].k[t]; }
        else if (A.dom == D_IN) A.b = 0.05 * (double)E.u(9) - 0.2;
        else { A.a = kDom[A.dom].s[t]; if (A.form == 9) A.c = kDom[A.dom].c[t]; else A.b = kDom[A.dom].c[t]; }
    }
}

void setter(Obj &o) {  // event 3
    switch (o.cls) {
        case OSC:
            mCount[M_PHASERESET]++;
            o.osc->phaseReset(o.family == 1 ? 1.0 + 500.0 * E.frac() : 0.001 + 0.99 * E.frac());
            break;
        case FLT:
            if (E.chance(1, 2)) { mCount[M_SETCUTOFF]++; o.p1 = shortLit(E, D_CUT); o.flt->setCutoff(o.p1); }
            else { mCount[M_SETRESONANCE]++; o.p2 = shortLit(E, D_RES); o.flt->setResonance(o.p2); }
            extra += 0.00001 * o.flt->getCutoff() + 0.01 * o.flt->getResonance();
            break;
        case ENV: {
            const double ms = 1 + (double)E.u(400);
            switch (E.u(6)) {
                case 0: mCount[M_SETATTACK]++; if (E.chance(1, 2)) o.env->setAttack(ms); else o.env->setAttackMS(ms); break;
                case 1: mCount[M_SETDECAY]++; o.env->setDecay(ms); break;
                case 2: mCount[M_SETSUSTAIN]++; o.env->setSustain(shortLit(E, D_UNIT)); break;
                case 3: mCount[M_SETRELEASE]++; o.env->setRelease(ms * 4); break;
                case 4: o.env->decay = 0.999 + 0.0001 * (double)E.u(9); o.env->holdtime = 1 + (long)E.u(300); break;
                default: o.env->setTrigger(1 - o.env->getTrigger()); break;
            }
            o.att = o.env->attack; o.dec = o.env->decay; o.sus = o.env->sustain; o.rel = o.env->release; o.hold = o.env->holdtime;
            break;
        }
        case SMP:
            if (E.chance(1, 2)) {
                mCount[M_TRIGGER]++;
                o.smp->trigger();
                o.posBound = 0;
            } else {
                mCount[M_SETPOSITION]++;
                const double p = 0.1 * (double)E.u(9) + 0.05 * E.frac();
                o.smp->setPosition(p);
                o.posBound = p * (double)dataLen(o) + 1.0;
            }
            break;
        case SVF:
            if (E.chance(1, 2)) { o.p1 = E.chance(1, 2) ? shortLit(E, D_CUT) : oddLit(E, D_CUT); o.svf->setCutoff(o.p1); }
            else { o.p2 = 0.5 + 0.5 * (double)E.u(9); o.svf->setResonance(o.p2); }
            mCount[M_SVFSET]++;
            break;
        case BIQ:
            o.itype = (int)E.u(7);
            o.p1 = shortLit(E, D_CUT);
            o.p2 = 0.5 + 0.25 * (double)E.u(12);
            applyParams(o);
            break;
        case EGN:
            if (E.chance(1, 3)) o.egn->setRetrigger(!o.egn->getRetrigger());
            else { o.p1 = 5 + (double)E.u(60); o.p2 = 20 + (double)E.u(100); applyParams(o); }
            break;
        default: changeLiteral(o, false); break;
    }
}

void memberAccess(Obj &o, int i) {  // event 4: a public state member read into the mix, another written -- every StateMember operator in turn
    if (o.cls != ENV) {
        if (o.cls == FLT) { extra += 0.00001 * o.flt->cutoff + 0.01 * o.flt->resonance; o.flt->cutoff += 1; }
        return;
    }
    maxiEnv &e = *o.env;
    mCount[M_ENVMEMBER]++;
    const unsigned op = memberOp++ % 8;
    opCount[op]++;
    const int j = peer(i);
    // half of the writes arrive BEFORE anything was read: the object still has a block rendered ahead then
    const bool writeFirst = E.chance(1, 2);
    for (int pass = 0; pass < 2; pass++) {
        if ((pass == 0) == writeFirst) {
            switch (op) {
                case 0: e.amplitude = 0.25; break;
                case 1: if (j >= 0) e.amplitude = objs[(size_t)j].env->amplitude; else e.amplitude = e.amplitude; break;
                case 2: e.amplitude += 0.125; break;
                case 3: e.amplitude -= 0.0625; break;
                case 4: e.amplitude *= 0.5; break;
                case 5: e.amplitude /= 3.0; break;
                case 6: ++e.holdcount; break;
                default: --e.holdcount; break;
            }
            if (E.chance(1, 4)) { e.attackphase = 1; e.releasephase = 0; }
            if (E.chance(1, 4)) e.holdcount = 0;
        } else {
            const double held = e.amplitude + e.output + e.holdcount + e.attackphase + e.decayphase + e.sustainphase + e.holdphase +
                                e.releasephase + e.input + e.holdtime;
            extra += 0.001 * clamp4(held * 0.01);
            opCount[8]++;
        }
    }
}

void copyMeta(Obj &dst, const Obj &src) {  // what an assigned object's bookkeeping inherits
    dst.att = src.att; dst.dec = src.dec; dst.sus = src.sus; dst.rel = src.rel; dst.hold = src.hold;
    dst.p1 = src.p1; dst.p2 = src.p2; dst.p3 = src.p3; dst.itype = src.itype; dst.loop = src.loop;
}
void copies(int i) {  // event 5
    Obj &o = objs[(size_t)i];
    const uint32_t what = E.u(4);
    if (what == 0) {  // a = b between live objects of one class
        const int j = peer(i);
        if (j < 0) return;
        Obj &b = objs[(size_t)j];
        if (o.cls == OSC && o.family != b.family) return;  // (phase families stay apart)
        if (o.cls == BIQ) return;                           // (the reference's maxiBiquad has a const member: not assignable)
        mCount[M_COPYASSIGN]++;
        switch (o.cls) {
            case OSC: *o.osc = *b.osc; break;
            case FLT: *o.flt = *b.flt; break;
            case ENV: *o.env = *b.env; break;
            case DLY: *o.dly = *b.dly; break;
            case SMP: *o.smp = *b.smp; o.data = b.data; o.posBound = 0; break;  // operator=: the samples, the head at 0
            case SVF: *o.svf = *b.svf; break;
            case DCB: *o.dcb = *b.dcb; break;
            case EGN: *o.egn = *b.egn; break;
            case FLG: *o.flg = *b.flg; break;
            default: *o.cho = *b.cho; break;
        }
        copyMeta(o, b);
    } else if (what == 1) {  // a temporary copy, called once and dropped
        mCount[M_COPYTEMP]++;
        Obj t;
        t.cls = o.cls;
        switch (o.cls) {
            case OSC: t.osc = new maxiOsc(*o.osc); break;
            case FLT: t.flt = new maxiFilter(*o.flt); break;
            case ENV: t.env = new maxiEnv(*o.env); break;
            case DLY: t.dly = new maxiDelayline(*o.dly); break;
            case SMP: t.smp = new maxiSample(*o.smp); break;
            case SVF: t.svf = new maxiSVF(*o.svf); break;
            case BIQ: t.biq = new maxiBiquad(*o.biq); break;
            case DCB: t.dcb = new maxiDCBlocker(*o.dcb); break;
            case EGN: t.egn = new maxiEnvGen(*o.egn); break;
            case FLG: t.flg = new maxiFlanger(*o.flg); break;
            default: t.cho = new maxiChorus(*o.cho); break;
        }
        double v[kMaxArgs] = {0, 0, 0, 0, 0};
        for (int k = 0; k < nArgs(o.cls); k++) {
            Arg A = o.arg[k];
            v[k] = evalArg(A);
        }
        if (o.cls == SMP && o.method == 2 && o.posBound + v[1] > (double)dataLen(o) - 4.0) v[1] = 0.25;
        extra += 0.05 * clamp4(callOn(o, v, t));
        destroy(t);
    } else if (what == 2) {  // a vector grows by a copy of a live object
        if (o.cls == OSC && o.family == 0 && vOsc.size() < 7) { vOsc.push_back(*o.osc); mCount[M_VECGROW]++; }
        else if (o.cls == ENV && vEnv.size() < 7) { vEnv.push_back(*o.env); mCount[M_VECGROW]++; }
        else if (o.cls == FLT && vFlt.size() < 7) { vFlt.push_back(*o.flt); mCount[M_VECGROW]++; }
    } else {
        if (o.cls == OSC && !vOsc.empty()) { vOsc.pop_back(); mCount[M_VECSHRINK]++; }
        else if (o.cls == ENV && !vEnv.empty()) { vEnv.erase(vEnv.begin()); mCount[M_VECSHRINK]++; }  // (the others move down: assignments)
        else if (o.cls == FLT && !vFlt.empty()) { vFlt.pop_back(); mCount[M_VECSHRINK]++; }
    }
}

void delayChange(Obj &o) {  // event 9
    if (E.chance(1, 2)) {
        o.arg[1].kind = A_LIT;
        o.arg[1].lit = (double)(1 + E.u(E.chance(1, 3) ? 40u : 3000u));
    } else {
        o.arg[2].kind = A_LIT;
        o.arg[2].lit = 0.05 * (double)E.u(19);
    }
    o.sinceChange = 0;
}

void event() {
    const int i = (int)E.u((uint32_t)objs.size());
    Obj &o = objs[(size_t)i];
    int kind = 1 + (int)E.u(9);
    if (kind == 9 && o.cls != DLY) {  // a delay line, if the graph has one
        int d = -1;
        for (size_t j = 0; j < objs.size(); j++)
            if (objs[j].cls == DLY && (d < 0 || E.chance(1, 2))) d = (int)j;
        if (d < 0) kind = 1 + (int)E.u(8);
        else {
            logEvent(9, d);
            delayChange(objs[(size_t)d]);
            return;
        }
    }
    logEvent(kind, i);
    switch (kind) {
        case 1: changeLiteral(o, E.chance(1, 2)); break;
        case 2: {
            drawMethod(o, E);
            if (o.cls == SMP) {  // the players keep their head in different ranges: start again from 0
                o.smp->trigger();
                o.posBound = 0;
            }
            break;
        }
        case 3: setter(o); break;
        case 4: {
            int e = i;
            if (o.cls != ENV && o.cls != FLT)
                for (size_t j = 0; j < objs.size(); j++)
                    if (objs[j].cls == ENV && (e == i || E.chance(1, 2))) e = (int)j;
            memberAccess(objs[(size_t)e], e);
            break;
        }
        case 5: copies(i); break;
        case 6:
            mCount[M_RECONSTRUCT]++;
            destroy(o);
            construct(o);
            o.sinceChange = 0;
            break;
        case 7:
            if (E.chance(1, 3)) { o.twice = true; mCount[M_TWICE]++; }
            else { o.skip = 1 + (int)E.u(E.chance(1, 2) ? 10u : 700u); mCount[M_SKIP]++; }
            break;
        case 8: {  // one member of a lock-step group gets event 1 or 3
            int g = -1;
            for (size_t j = 1; j < objs.size(); j++)
                if (objs[j].cls == objs[j - 1].cls && objs[j].method == objs[j - 1].method && (g < 0 || E.chance(1, 2))) g = (int)j;
            if (g < 0) g = i;
            if (E.chance(1, 2)) changeLiteral(objs[(size_t)g], E.chance(1, 2)); else setter(objs[(size_t)g]);
            break;
        }
        default: delayChange(o); break;
    }
}

}  // namespace

void setup() {
    const char *e;
    uint64_t seed = 1;
    if ((e = std::getenv("MXG_FUZZ_SEED"))) seed = (uint64_t)std::strtoull(e, nullptr, 10);
    if ((e = std::getenv("MXG_FUZZ_PROFILE"))) profile = std::atoi(e) & 3;
    if ((e = std::getenv("MXG_FUZZ_FRAMES"))) totalFrames = std::atol(e);
    if ((e = std::getenv("MXG_FUZZ_LOG"))) logEvents = e[0] == '1';
    int maxObj = 24;
    if ((e = std::getenv("MXG_FUZZ_MAXOBJ"))) maxObj = std::atoi(e);
    static const size_t bufs[4] = {512, 64, 1024, 512};
    maxiSettings::setup(44100, 2, bufs[profile]);
    G.s = (seed + 1) * 0x9E3779B97F4A7C15ull + (uint64_t)profile * 0xD1B54A32D192ED03ull;
    if (!G.s) G.s = 1;
    for (int k = 0; k < 8; k++) G.next();
    E.s = G.next() | 1;
    uint64_t l = G.next() | 1;
    sampleData[0].resize(4096);
    sampleData[1].resize(3000);
    for (int d = 0; d < 2; d++)
        for (size_t k = 0; k < sampleData[d].size(); k++) {
            l = l * 6364136223846793005ull + 1442695040888963407ull;
            sampleData[d][k] = ((double)(int)((l >> 40) % 2001) - 1000.0) / 1250.0;
        }
    int n = 8 + (int)G.u(17);
    if (n > maxObj) n = maxObj;
    if (n < 1) n = 1;
    const int groupDen = profile == 1 ? 3 : 8;
    int fx = 0;
    while ((int)objs.size() < n) {
        const int self = (int)objs.size();
        int cls = self == 0 ? (int)OSC : pickClass();
        if (cls == FLG || cls == CHO) {
            if (fx >= 2) cls = DLY;
            fx++;
        }
        Obj o = drawObject(cls, self);
        objs.push_back(o);
        if (cls != FLG && cls != CHO && cls != DLY && G.chance(1, (uint32_t)groupDen)) {  // a lock-step group: equal arguments, one loop
            mCount[M_GROUPS]++;
            const int members = 1 + (int)G.u(7);
            for (int m = 0; m < members && (int)objs.size() < n; m++) {
                Obj c = o;
                c.w = o.w * 0.5;
                objs.push_back(c);
            }
        }
    }
    for (Obj &o : objs) construct(o);
    std::atexit(report);
}

void play(double *output) {
    extra = 0;
    if (eventsOn()) {
        const uint32_t den = profile == 1 ? 30u : (profile == 2 ? 45u : 40u);
        if (E.chance(1, den)) event();
    }
    double mix = 0;
    for (size_t i = 0; i < objs.size(); i++) {
        Obj &o = objs[i];
        if (o.cls == DLY && eventsOn()) {  // the block edges: just before, on and after 8, 64 and 512 calls since the last change
            const long c = o.sinceChange;
            const bool edge = (c >= 7 && c <= 9) || (c >= 63 && c <= 65) || (c >= 511 && c <= 513);
            if (edge && E.chance(1, profile == 2 ? 3u : 6u)) {
                logEvent(9, (int)i);
                delayChange(o);
            }
        }
        if (o.skip > 0) {
            o.skip--;
        } else {
            double v[kMaxArgs] = {0, 0, 0, 0, 0};
            for (int k = 0; k < nArgs(o.cls); k++) v[k] = evalArg(o.arg[k]);
            o.out = callOn(o, v, o);
            if (o.twice) {
                o.twice = false;
                o.out = callOn(o, v, o);
                if (o.cls == DLY) o.sinceChange++;
            }
            if (o.cls == DLY) o.sinceChange++;
        }
        mix += o.w * o.out;
    }
    // the vectors' elements: fixed arguments, a loop each
    for (size_t k = 0; k < vOsc.size(); k++) mix += 0.02 * vOsc[k].phasor(3 + (double)k);
    const int gate = (frame % 2000) < 700;
    for (size_t k = 0; k < vEnv.size(); k++) mix += 0.02 * vEnv[k].adsr(1.0, 0.01, 0.9995, 0.4, 0.9997, 100, gate);
    for (size_t k = 0; k < vFlt.size(); k++) mix += 0.02 * vFlt[k].lores(clamp4(objs[0].out), 1000, 2);
    output[0] = mix + extra;
    output[1] = objs[(size_t)frame % objs.size()].out;
    for (Obj &o : objs) o.prev = o.out;
    frame++;
}
