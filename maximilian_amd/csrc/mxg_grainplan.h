// mxg_grainplan.h -- what a mxg_grain_plan holds (grains.hip creates and destroys it; grainpool.hip reads it).
#pragma once
#include <vector>

struct mxg_grain_plan {
    int window_kind, mySampleRate;
    double grainLength;
    unsigned long sampleDur;
    double *d_window;  // [sampleDur]
    std::vector<double> h_window;
};
