// include/libs/maxiPolyBLEP.h -- the reference keeps maxiPolyBLEP under src/libs/: patches that include "libs/maxiPolyBLEP.h"
// find maxiPolyBLEP in the drop-in header.
#pragma once
#include "../maxiPolyBLEP.h"
