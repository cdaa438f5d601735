// include/maxiClock.h -- DROP-IN for the reference's metronome maxiClock (src/libs/maxiClock.h, maxiClock.cpp): a plain host class,
// as in the reference, whose `timer` is the drop-in maxiOsc -- so the phase it counts on is the per-sample engine's phasor, the
// reference's bits.  ticker(): tick = false; currentCount = floor(timer.phasor(bps)); if (lastCount != currentCount) { tick = true;
// playHead++; } -- ticker never writes lastCount, so with lastCount 0 a tick is the one sample per wrap on which the phasor returns
// a phase >= 1.  Banks of clocks run on the device: maxiClockBank (include/maximilian_bank.hpp, mxg_clock_render).
#pragma once
#include "maximilian.h"

class maxiClock {
public:
    maxiClock() {  // maxiClock.cpp:4-13
        playHead = 0;
        currentCount = 0;
        lastCount = 0;
        bpm = 120;
        ticks = 1;
        setTempo(bpm);
    }
    void ticker() {  // maxiClock.cpp:16-28
        tick = false;
        currentCount = (int)floor(timer.phasor(bps));
        if (lastCount != currentCount) {
            tick = true;
            playHead++;
        }
    }
    void setTempo(double bpmIn) {  // maxiClock.cpp:31-35
        bpm = bpmIn;
        bps = (bpm / 60.) * ticks;
    }
    void setTicksPerBeat(int ticksPerBeat) {  // maxiClock.cpp:38-43
        ticks = ticksPerBeat;
        setTempo(bpm);
    }
    maxiOsc timer;
    int currentCount;
    int lastCount;
    int playHead;
    double bps;
    double bpm;
    int ticks;
    bool tick = false;

    // the reference's get / set pairs over the public members above (its int parameters for bps, bpm and tick included)
    void setCurrentCount(int n) { currentCount = n; }
    int getCurrentCount() const { return currentCount; }
    void setLastCount(int n) { lastCount = n; }
    int getLastCount() const { return lastCount; }
    void setPlayHead(int n) { playHead = n; }
    int getPlayHead() const { return playHead; }
    void setBps(int v) { bps = v; }
    double getBps() const { return bps; }
    void setBpm(int v) { bpm = v; }
    double getBpm() const { return bpm; }
    void setTicks(int v) { ticks = v; }
    int getTicks() const { return ticks; }
    void setTick(int v) { tick = v != 0; }
    bool getTick() const { return tick; }
    int isTick() const { return tick ? 1 : 0; }
};
