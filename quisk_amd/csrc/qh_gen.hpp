// qh_gen.hpp -- xgen as RXA's gen0 runs it (wdsp/gen.c:173-354, RXA.c:565): a running generator REPLACES the channel's buffer behind
// xresample with a tone, two tones, noise, a sweep, a keyed pulse or silence.  One launch writes the rows of the listed channels; every
// sample is computed for itself from the channel's state at the start of the call, and a small launch behind it moves the running
// mode's state on by the call's length, on the device, so that a replayed launch sequence (which bakes in its kernels' arguments)
// carries on like the plain path.  Modes 4 and 5 (sawtooth, triangle) are refused by the engine (chain_needs).
//
// Tone, two-tone and the pulse's 1 kHz carrier: the reference re-seeds cos / sin from `phs` at the top of a block and rotates per sample,
// and walks `phs += delta` wrapped into [0, 2 pi); here sample i is sincos(phs + i delta) and the state moves by n delta, wrapped.
// Sweep: `phs += dphs; dphs += d2phs` per sample with dphs reset every P samples.  P is the reference's own count (qh_design.cpp,
// sweep_walk), and so is the table of (phs, dphs) every kGenCkStep samples of a period: `dphs += d2phs` rounds by the same amount at every
// step inside a binade of dphs, so the reference's dphs runs off the exact line by up to half an ulp a step and its phase off the exact
// quadratic by 1e-5 rad over the default period.  From a table entry on the quadratic is exact to 3e-8 rad.
// Pulse: the position in the period pnoff + 2 pntrans + pnon is an integer; a negative one is flush_gen's quirk (OFF with the count of
// another state left over, gen.c:160-163).
// Noise: Marsaglia's polar method as in gen.c:232-243 on a counter-based uniform source (the reference's is rand()): see gen_noise.
#pragma once
#include <hip/hip_runtime.h>
#include "qh_kernels.hpp"

namespace qh {

static constexpr int kGenCkShift = 14, kGenCkStep = 1 << kGenCkShift;          // sweep table: one entry every 16384 samples of a period
static constexpr long long kGenWalkMax = 1LL << 27;                            // additions sweep_walk makes at most
static constexpr int kGenCkMax = (int)(kGenWalkMax >> kGenCkShift) + 2;        // entries per channel
static constexpr double kGenTwoPi = 6.2831853071795864;                        // TWOPI, comm.h
static constexpr unsigned long long kGenGolden = 0x9E3779B97F4A7C15ull;
static constexpr int kGenNoiseAttempts = 64;                                   // (an attempt is rejected with probability 1 - pi / 4)

struct GenParam {               // per channel, uploaded when a setter changed it
    int mode, pntrans, pnon, pnoff;
    int sweep_nck, pad;         // table entries in use; 0: one quadratic from the period's start (P beyond the walk's cap, or no reset)
    long long sweep_P;          // samples between resets, 0: never
    double tone_mag, tone_delta;
    double tt_mag1, tt_mag2, tt_delta1, tt_delta2;
    double noise_mag;
    unsigned long long noise_key;       // mix64(seed + golden (ch + 1))
    double sweep_mag, sweep_dphs0, sweep_d2phs, sweep_full;     // full: the phase a whole period adds, wrapped
    double pulse_mag, pulse_tdelta;
};

struct GenState {               // per channel, lives and moves on the device; all zero as create_gen leaves it
    double tone_phs, tt_phs1, tt_phs2, pulse_tphs;
    long long pulse_pos;                // position in the pulse's period; < 0: OFF for that many samples more than pnoff
    unsigned long long noise_ctr;       // noise samples drawn so far
    double sweep_phs;                   // phase at the start of the current period (P > 0) or of the call (P == 0)
    long long sweep_pos;                // samples since the last reset (P > 0) or since calc_sweep (P == 0)
};

__host__ __device__ static inline unsigned long long gen_mix64(unsigned long long z)      // splitmix64's finalizer
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ static inline double gen_wrap(double x)      // into [0, 2 pi)
{
    x -= kGenTwoPi * floor(x / kGenTwoPi);
    if (x >= kGenTwoPi) x -= kGenTwoPi;
    if (x < 0.0) x += kGenTwoPi;
    return x;
}

// Sample `ctr` of a channel's noise stream: r = 2 u - 1 with u the top 53 bits of a 64-bit word, the words of attempt a being
// mix64(K + golden (2 a + 1)) and mix64(K + golden (2 a + 2)), K = mix64(key + golden ctr).  c >= 1.0 is rejected as in the reference (and
// c == 0, whose logarithm it would take); the products and the sum are rounded one by one so that a host restatement decides alike.
__device__ static inline double2 gen_noise(unsigned long long key, unsigned long long ctr, double mag)
{
    const unsigned long long K = gen_mix64(key + kGenGolden * ctr);
    for (int a = 0; a < kGenNoiseAttempts; a++) {
        const unsigned long long w1 = gen_mix64(K + kGenGolden * (unsigned long long)(2 * a + 1));
        const unsigned long long w2 = gen_mix64(K + kGenGolden * (unsigned long long)(2 * a + 2));
        const double r1 = 2.0 * ((double)(w1 >> 11) * 0x1p-53) - 1.0;         // exact, fused or not
        const double r2 = 2.0 * ((double)(w2 >> 11) * 0x1p-53) - 1.0;
        double c;
        {
#pragma clang fp contract(off)
            const double s1 = r1 * r1, s2 = r2 * r2;
            c = s1 + s2;
        }
        if (c >= 1.0 || c == 0.0) continue;
        const double rad = sqrt(-2.0 * log(c) / c);
        return make_double2(mag * rad * r1, mag * rad * r2);
    }
    return make_double2(0.0, 0.0);
}

// The sweep's phase r samples into a period, less the phase at the period's start
__device__ static inline double gen_sweep_phase(const GenParam &p, const double2 *ck, long long r)
{
    double ph = 0.0, dphs = p.sweep_dphs0;
    long long t = r;
    if (p.sweep_nck > 0) {
        long long j = r >> kGenCkShift;
        if (j >= p.sweep_nck) j = p.sweep_nck - 1;
        const double2 e = ck[j];
        ph = e.x; dphs = e.y; t = r - (j << kGenCkShift);
    }
    const double td = (double)t;
    return ph + td * dphs + p.sweep_d2phs * (0.5 * td * (td - 1.0));
}

// the rows of the listed channels, n samples each
static __global__ __launch_bounds__(NT) void gen_kernel(double2 *buf, long long stride, int n, const int *chan_list, const GenParam *prm,
                                                        const GenState *state, const double2 *sweep_ck, const double *ctrans)
{
    const int ch = chan_list[blockIdx.y];
    const GenParam p = prm[ch];
    const GenState s = state[ch];
    double2 *row = buf + (long long)ch * stride;
    const double2 *ck = sweep_ck + (long long)ch * kGenCkMax;
    const long long T = (long long)p.pnoff + 2LL * p.pntrans + p.pnon;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {      // (n may be near 2^31)
        double2 v = make_double2(0.0, 0.0);
        double sn, cs;
        switch (p.mode) {
        case 0:
            sincos(s.tone_phs + (double)i * p.tone_delta, &sn, &cs);
            v = make_double2(p.tone_mag * cs, -p.tone_mag * sn);
            break;
        case 1: {
            double s2, c2;
            sincos(s.tt_phs1 + (double)i * p.tt_delta1, &sn, &cs);
            sincos(s.tt_phs2 + (double)i * p.tt_delta2, &s2, &c2);
            v = make_double2(p.tt_mag1 * cs + p.tt_mag2 * c2, -p.tt_mag1 * sn - p.tt_mag2 * s2);
            break;
        }
        case 2:
            v = gen_noise(p.noise_key, s.noise_ctr + (unsigned long long)i, p.noise_mag);
            break;
        case 3: {
            const long long q = s.sweep_pos + i;
            double ph;
            if (p.sweep_P > 0) {
                const long long m = q / p.sweep_P, r = q - m * p.sweep_P;
                ph = s.sweep_phs + (double)m * p.sweep_full + gen_sweep_phase(p, ck, r);
            } else {        // no reset: the quadratic of this call, from the dphs the chain has reached
                const double d = p.sweep_dphs0 + (double)s.sweep_pos * p.sweep_d2phs, td = (double)i;
                ph = s.sweep_phs + td * d + p.sweep_d2phs * (0.5 * td * (td - 1.0));
            }
            sincos(ph, &sn, &cs);
            v = make_double2(p.sweep_mag * cs, -p.sweep_mag * sn);
            break;
        }
        case 6: {
            if (p.pnoff == 0) break;                    // gen.c:296,332-333
            long long pos = s.pulse_pos + i;
            if (pos < 0) break;                         // OFF
            pos %= T;
            if (pos < p.pnoff) break;                   // OFF
            pos -= p.pnoff;
            double g;
            if (pos < p.pntrans) g = ctrans[pos];                                               // UP: ctrans[pntrans - pcount]
            else if (pos < (long long)p.pntrans + p.pnon) g = 1.0;                              // ON
            else g = ctrans[p.pntrans - (pos - p.pntrans - p.pnon)];                            // DOWN: ctrans[pcount]
            cs = cos(s.pulse_tphs + (double)i * p.pulse_tdelta);
            v.x = g == 1.0 ? p.pulse_mag * cs : p.pulse_mag * cs * g;
            break;
        }
        default:
            break;
        }
        row[i] = v;
    }
}

// the running mode's state of the listed channels, n samples on; behind gen_kernel on its stream
static __global__ void gen_advance_kernel(int n, const int *chan_list, int count, const GenParam *prm, GenState *state)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int ch = chan_list[k];
    const GenParam p = prm[ch];
    GenState s = state[ch];
    const double dn = (double)n;
    switch (p.mode) {
    case 0: s.tone_phs = gen_wrap(s.tone_phs + dn * p.tone_delta); break;
    case 1: s.tt_phs1 = gen_wrap(s.tt_phs1 + dn * p.tt_delta1); s.tt_phs2 = gen_wrap(s.tt_phs2 + dn * p.tt_delta2); break;
    case 2: s.noise_ctr += (unsigned long long)n; break;
    case 3:
        if (p.sweep_P > 0) {
            const long long q = s.sweep_pos + n, m = q / p.sweep_P;
            s.sweep_pos = q - m * p.sweep_P;
            if (m) s.sweep_phs = gen_wrap(s.sweep_phs + (double)m * p.sweep_full);
        } else {
            const double d = p.sweep_dphs0 + (double)s.sweep_pos * p.sweep_d2phs;
            s.sweep_phs = gen_wrap(s.sweep_phs + dn * d + p.sweep_d2phs * (0.5 * dn * (dn - 1.0)));
            s.sweep_pos += n;
        }
        break;
    case 6: {
        s.pulse_tphs = gen_wrap(s.pulse_tphs + dn * p.pulse_tdelta);
        if (p.pnoff != 0) {
            const long long T = (long long)p.pnoff + 2LL * p.pntrans + p.pnon;
            s.pulse_pos += n;
            if (s.pulse_pos >= 0) s.pulse_pos %= T;
        }
        break;
    }
    default: break;
    }
    state[ch] = s;
}

// flush_gen (gen.c:160-163) for every channel: the state goes to OFF and pcount, the samples the state it was in had left, stays -- OFF
// then lasts that long, which is position pnoff - pcount
static __global__ void gen_flush_kernel(int nch, const GenParam *prm, GenState *state)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    const GenParam p = prm[ch];
    const long long pos = state[ch].pulse_pos, up = p.pnoff, on = up + p.pntrans, down = on + p.pnon, T = down + p.pntrans;
    if (pos < up) return;                // OFF already
    const long long left = (pos < on ? on : pos < down ? down : T) - pos;
    state[ch].pulse_pos = (long long)p.pnoff - left;
}

}  // namespace qh
