// the thread-per-pair kernels of a super-step for the horizon N = 30 (BASELINE configs[4], the closed loop): bmpc_pair_fixed.hpp
#define BMPC_FIXED_N 30
#include "bmpc_pair_fixed.hpp"
