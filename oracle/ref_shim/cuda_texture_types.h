// REFERENCE PIN stand-in: see cuda_runtime.h
#include "cuda_runtime.h"
