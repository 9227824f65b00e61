// CPU definitions of the platform names the device code is written against -- the counterpart of
// boundplanner_amd/csrc/bmpc_platform_hip.hpp for the emulator builds (TEST INFRASTRUCTURE ONLY).  One lane, one workgroup, no
// barrier: what the thread-per-instance bodies (bmpc_loop.hpp, bmpc_ik.hpp, bmpc_sets.hpp) need.  emu_pipe.cpp, which runs the
// lanes of a wavefront as threads, defines BMPC_SYNC / BMPC_FENCE_SYNC / BMPC_LANE (and its atomic counter increment) itself
// before it includes this header.
#pragma once
#include <cmath>

#define BMPC_DEV inline
#define BMPC_INL inline
#define BMPC_KBODY inline
#define BMPC_HD inline
#define BMPC_NOINL
#define BMPC_AS1
typedef double LDSD;
typedef double bmpc_v2d __attribute__((vector_size(16)));
typedef bmpc_v2d LDSV2;
#ifndef BMPC_SYNC
#define BMPC_SYNC() do {} while (0)
#endif
#ifndef BMPC_FENCE_SYNC
#define BMPC_FENCE_SYNC() do {} while (0)
#endif
#ifndef BMPC_LANE
#define BMPC_LANE() 0
#endif
#define BMPC_NT 64
#define BMPC_BLOCK() 0
#define BMPC_NBLOCKS() 1
#define BMPC_PIN(x) do {} while (0)
#define BMPC_UNIFORM(x) (x)
#define BMPC_OPAQUE_I(x) do {} while (0)
#define BMPC_TOUCH_LINE(g, l) do {} while (0)
#define BMPC_SCHED_FENCE() do {} while (0)
#define BMPC_ASYNC_WAIT() do {} while (0)
#define BMPC_RSQRT(x) (1.0 / std::sqrt(x))
#define BMPC_RCP(x) (1.0 / (x))
#define BMPC_MUL24(a, b) ((a) * (b))
#define BMPC_SINCOS(x, s, c) do { (s) = std::sin(x); (c) = std::cos(x); } while (0)
#define BMPC_LDS_ADD(ptr, v) (*(ptr) += (v))
using std::fmax;
using std::fmin;

// the LDS-DMA copy of bmpc_platform_hip.hpp as plain loads and stores, same chunk-to-wavefront assignment
template <int NCH, int NT> static inline void bmpc_async_copy(const double* gsrc, double* lds_dst, int lane) {
    const int wave = lane >> 6, wl = lane & 63;
    for (int i = 0; i < (NCH + NT / 64 - 1) / (NT / 64); i++) {
        const int c = i * (NT / 64) + wave;
        if (c < NCH) { lds_dst[128 * c + 2 * wl] = gsrc[128 * c + 2 * wl]; lds_dst[128 * c + 2 * wl + 1] = gsrc[128 * c + 2 * wl + 1]; }
    }
}
