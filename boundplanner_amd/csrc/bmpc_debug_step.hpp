// What is wrong with the arguments of bmpc_debug_superstep (include/boundmpc.h), or null: the one statement of which fields of the
// record go together, for the entry (bmpc_capi.hip) and for the CPU emulation of its sequence (tests/emu/emu_pipe.cpp).  Host code;
// what depends on the handle (hess, trial_repeats, the workspace slots) is the entry's own business.
#pragma once
#include "../../include/boundmpc.h"

inline const char* bmpc_debug_step_refusal(int B, const bmpc_debug_step* s) {
    if (B <= 0 || !s || !s->x0 || !s->lbx || !s->ubx || !s->p) return "bad argument";
    const int n_rows = !!s->t + !!s->z + !!s->mode, n_newton = !!s->dzeta + !!s->dt + !!s->dz + !!s->state;
    const int n_trial = !!s->zeta0 + !!s->t0 + !!s->z0 + !!s->zeta1 + !!s->t1 + !!s->z1 + !!s->ls;
    if (n_rows % 3) return "t, z and mode are given together or not at all";
    if (!n_rows && (s->plant0 || s->plant1 || s->ctl_plant)) return "state is planted with given rows only";
    if (s->mode) for (int i = 0; i < B; i++) if (s->mode[i] < 0 || s->mode[i] > 2) return "mode must be 0, 1 or 2";
    if (s->H ? n_newton || n_trial || s->ctl : n_newton != 4 || n_trial % 7) return "H alone, or dzeta, dt, dz, state with all or none of the trial outputs";
    if (s->H ? !s->lam_pi || !n_rows : s->lam_pi != nullptr) return "H needs t, z and lam_pi, and nothing else takes lam_pi";
    if (!n_trial && (s->plant0 || s->plant1 || s->ctl_plant || s->ctl)) return "plant0, plant1, ctl_plant and ctl go with the trial outputs";
    return nullptr;
}
