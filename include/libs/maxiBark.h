// include/libs/maxiBark.h -- the reference keeps maxiBark under src/libs/: patches that include "libs/maxiBark.h" find
// maxiBarkScaleAnalyser / maxiBark in the drop-in header.
#pragma once
#include "../maxiBark.h"
