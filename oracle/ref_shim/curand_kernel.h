// Stand-in for the system header of this name (see cuda_runtime.h here): the reference's device code only needs it to exist.
#pragma once
#include "cuda_runtime.h"
