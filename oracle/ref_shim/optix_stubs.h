// Stand-in for the system header of this name: the OptiX device calls live in optix.h here.
#pragma once
#include "optix.h"
