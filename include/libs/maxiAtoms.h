// include/libs/maxiAtoms.h -- the reference keeps maxiAtoms under src/libs/: patches that include "libs/maxiAtoms.h" find its classes
// in the drop-in header.
#pragma once
#include "../maxiAtoms.h"
