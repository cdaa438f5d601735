// include/libs/maxiClock.h -- the reference keeps maxiClock under src/libs/: patches that include "libs/maxiClock.h" find maxiClock in
// the drop-in header.
#pragma once
#include "../maxiClock.h"
