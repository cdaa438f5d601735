// include/libs/maxiReverb.h -- the reference keeps its reverbs under src/libs/: patches that include "libs/maxiReverb.h" find
// maxiSatReverb / maxiFreeVerb / maxiFreeVerbStereo / maxiDattaroReverb in the drop-in header.
#pragma once
#include "../maxiReverb.h"
