// include/libs/maxim.h -- the reference's umbrella header for its analysis classes (src/libs/maxim.h): patches that include it
// next to "maximilian.h" (e.g. maximilian_examples/20.FFT_example) find maxiFFT / maxiIFFT / maxiMFCC / maxiFFTOctaveAnalyzer in
// the drop-in header, and maxiBark and the atoms classes (maxiAtoms.h) as the reference's maxim.h provides them.
#pragma once
#include "../maximilian.h"
#include "../maxiBark.h"
#include "../maxiAtoms.h"
