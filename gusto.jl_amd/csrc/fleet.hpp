// fleet.hpp -- the argument check of the fleet stage (fleet.hip), a pure host function: no device, no handle, nothing of HIP.
// tests/c/fleet_args.cpp compiles it into a host program.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "gusto_hip.h"

// J_b = (int)ceil(tf / h) + 1 as a double (so that a NaN or an overflow is seen before the cast)
static inline double fleet_clock_samples(double tf, double h) { return ceil(tf / h) + 1.0; }

// The arguments of gusto_fleet_schedule / gusto_fleet_separation behind the handle's own refusals (TrajOpt), in the order of
// include/gusto_hip.h: the model, R, the options, order [B] (null: index order), delay_steps [B] (null: none given), then the
// clock: tf [B] (null: not looked at -- the entry checks it once tf is back from the device) with *J_max the largest J_b.
// GUSTO_ERR_ARG and the text, which names the first offending fleet or problem, in *err.
static inline int fleet_args_host(int model, int B, int R, const gusto_fleet_opts* o, const int* order, const int* delay_steps,
                                  const double* tf, int* J_max, const char* who, std::string* err) {
    const std::string w = std::string(who) + ": ";
    if (model == GUSTO_DUBINS_CAR) { *err = w + "DubinsCar cannot hold at its start and has no robot geometry"; return GUSTO_ERR_ARG; }
    if (R < 1 || R > GUSTO_MAX_STARTS) { *err = w + "R outside 1 .. GUSTO_MAX_STARTS"; return GUSTO_ERR_ARG; }
    if (B < 1 || B % R != 0) { *err = w + "R does not divide B"; return GUSTO_ERR_ARG; }
    if (!(o->dt_clock > 0 && o->dt_clock < INFINITY)) { *err = w + "dt_clock must be positive and finite"; return GUSTO_ERR_ARG; }
    if (!(o->margin >= 0 && o->margin < INFINITY)) { *err = w + "margin must be finite and >= 0"; return GUSTO_ERR_ARG; }
    if (o->n_delays < 1 || o->n_delays > 64) { *err = w + "n_delays outside 1 .. 64"; return GUSTO_ERR_ARG; }
    if (o->delay_stride < 1 || o->delay_stride > GUSTO_FLEET_MAX_SHIFT / 64) { *err = w + "delay_stride outside 1 .. GUSTO_FLEET_MAX_SHIFT / 64"; return GUSTO_ERR_ARG; }
    if (o->clock_cap < 2 || o->clock_cap > GUSTO_FLEET_MAX_SHIFT) { *err = w + "clock_cap outside 2 .. GUSTO_FLEET_MAX_SHIFT"; return GUSTO_ERR_ARG; }
    if (o->components != 0 && o->components != 1) { *err = w + "components must be 0 or 1"; return GUSTO_ERR_ARG; }
    if (o->prune != 0 && o->prune != 1) { *err = w + "prune must be 0 or 1"; return GUSTO_ERR_ARG; }
    for (int f = 0; order && f < B / R; f++) {
        unsigned long long seen = 0;
        for (int p = 0; p < R; p++) {
            const int i = order[(size_t)f * R + p];
            if (i < 0 || i >= R || (seen >> i & 1)) { *err = w + "order is not a permutation of 0 .. R - 1 (fleet " + std::to_string(f) + ")"; return GUSTO_ERR_ARG; }
            seen |= 1ull << i;
        }
    }
    for (int b = 0; delay_steps && b < B; b++)
        if (delay_steps[b] < -1 || delay_steps[b] > GUSTO_FLEET_MAX_SHIFT) {
            *err = w + "delay_steps outside -1 .. GUSTO_FLEET_MAX_SHIFT (problem " + std::to_string(b) + ")";
            return GUSTO_ERR_ARG;
        }
    if (J_max) *J_max = 0;
    for (int b = 0; tf && b < B; b++) {
        const double J = fleet_clock_samples(tf[b], o->dt_clock);
        if (!(tf[b] > 0 && J >= 2 && J <= (double)o->clock_cap)) {
            *err = w + "problem " + std::to_string(b) + " needs ceil(tf / dt_clock) + 1 = " + std::to_string(J) + " clock samples, outside 2 .. clock_cap";
            return GUSTO_ERR_ARG;
        }
        if (J_max && (int)J > *J_max) *J_max = (int)J;
    }
    return GUSTO_OK;
}
