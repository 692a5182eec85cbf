// qh_varsamp.hpp -- the control recurrence of WDSP's variable-ratio resampler (xvarsamp, wdsp/varsamp.c:124-179) as one function that
// compiles as host code and as device code (qh_varsamp.hip runs it one lane per channel; tests/test_design_varsamp_host.py compiles it
// with g++).  It reads no samples: from a channel's state, the call's n and var it says at which input sample every output sample is
// made and which h_offset is in force there.
//
// Every statement is the reference's, in its order, in IEEE doubles.  There is no sum of a product in it that a compiler could contract
// into a fused multiply-add, and the one division per call is the correctly rounded one on both sides (never build this with
// fast-math): host and device give the same bits, which is what makes the output counts exact.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define QH_VS_HD __host__ __device__
#else
#define QH_VS_HD
#endif

namespace qh {

// what xvarsamp keeps from call to call, but for the ring: varsamp.c:129-132,158-160,170-172
struct VarsampState {
    double inv_cvar, h_offset, isamps;
    double var;                         // the var of the last call (a->var): calc_varsamp starts inv_cvar over from it
};

QH_VS_HD inline double varsamp_clear16(double v)        // varsamp.c:149-151
{
    uint64_t N;
    __builtin_memcpy(&N, &v, sizeof N);
    N &= 0xffffffffffff0000ull;
    __builtin_memcpy(&v, &N, sizeof v);
    return v;
}

// One call of xvarsamp on the state `s`: emit(m, i, h_offset) for output sample m = 0, 1, ..., made when input sample i of the call is the
// newest one in the ring, with the h_offset hshift sees (varsamp.c:157, before the step of :158-160).  Returns the count.  run = 0: the
// entry statements alone (varsamp.c:129-138 stand in front of `if (a->run)`), and n is returned (the copy of :176-177).
// n = 0: the quotient of varsamp.c:135 is not formed (it is never used: the loop does not run, and :136 stores old_inv_cvar).
template <typename Emit>
QH_VS_HD inline int varsamp_walk(VarsampState &s, int n, double var, double nom_ratio, int varmode, int run, Emit emit)
{
    int outsamps = 0;
    s.var = var;                                                    // :129
    const double old_inv_cvar = s.inv_cvar;                         // :130
    const double cvar = var * nom_ratio;                            // :131
    double inv_cvar = 1.0 / cvar;                                   // :132
    double dicvar = 0.0;                                            // :138
    if (varmode) {
        if (n > 0) dicvar = (inv_cvar - old_inv_cvar) / (double)n;  // :135
        inv_cvar = old_inv_cvar;                                    // :136
    }
    if (!run) {
        s.inv_cvar = inv_cvar;
        return n;
    }
    double h_offset = s.h_offset, isamps = s.isamps;
    for (int i = 0; i < n; i++) {                                   // :144
        inv_cvar += dicvar;                                         // :148
        inv_cvar = varsamp_clear16(inv_cvar);                       // :149-151
        const double delta = 1.0 - inv_cvar;                        // :152
        while (isamps < 1.0) {                                      // :153
            emit(outsamps, i, h_offset);                            // hshift, :157, and the dot product of :161-168
            h_offset += delta;                                      // :158
            while (h_offset >= 1.0) h_offset -= 1.0;                // :159
            while (h_offset < 0.0) h_offset += 1.0;                 // :160
            outsamps++;                                             // :169
            isamps += inv_cvar;                                     // :170
        }
        isamps -= 1.0;                                              // :172
    }
    s.inv_cvar = inv_cvar;
    s.h_offset = h_offset;
    s.isamps = isamps;
    return outsamps;
}

}  // namespace qh
