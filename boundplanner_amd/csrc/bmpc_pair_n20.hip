// the thread-per-pair kernels of a super-step for the horizon N = 20 (BASELINE configs[2], the benchmark): bmpc_pair_fixed.hpp
#define BMPC_FIXED_N 20
#include "bmpc_pair_fixed.hpp"
