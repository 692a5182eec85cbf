// qh_audio_peak.hpp -- xcbl -> xspeak -> xmpeak of xrxa (wdsp/RXA.c:591-593): the carrier block (cblock.c:74-94), the CW audio peak
// filter (iir.c:265-296, design 1, four stages) and the two-tone peak filter (iir.c:439-460), per listed channel, in place on the
// engine's rows at dsp rate, state carried from call to call.
//
// All three are linear recurrences run on I and Q alike, so the call is cut into time tiles of L samples, one tile per lane
// (pll_lanes_kernel's form, qh_tiled.hpp), in three launches:
//   pass 0  every tile but the last runs from the zero state and leaves its end state e_j           (one read of the rows)
//   carry   s_{j+1} = T s_j + e_j over the tiles of a channel in order, T = A^L the state's transition over a tile with zero input
//           (A built on the host by stepping the unit states through ap_step, T by squaring): every tile's start state
//   pass 1  every tile runs from its start state and writes its samples back; the last tile leaves the channel's state
//           (one read and one write of the rows)
// State per component (kApDim = 32 doubles): the blocker's previous input and output, then per cascade (speak, peak 0, peak 1) the
// first stage's x1, x2 and every stage's y1, y2 -- a later stage's x1, x2 are the stage before's y1, y2, so they are not kept twice.
// A stage that does not run (run 0, a disabled peak, a peak at or past npeaks) neither steps nor moves: its rows of A are the
// identity and its share of e_j is zero, so its state stands still across the call, as the reference's does.
// Inside a tile the reference's recurrence is stepped as written, the blocker's 1e-100 flush included; at a tile start the carried
// output gets the same flush (the carry itself is linear).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace qh {

static constexpr int kApPeaks = 2;                              // create_rxa's mpeak holds two peaks (RXA.c:427-445)
static constexpr int kApStages = 4;                             // nstages of speak and of every peak (RXA.c:414-445)
static constexpr int kApCascade = 2 + 2 * kApStages;            // x1, x2 of the first stage; y1, y2 of every stage
static constexpr int kApDim = 2 + kApCascade * (1 + kApPeaks);  // per component: 32
static constexpr int kApW = 2 * kApDim;                         // I then Q: one channel's state, one tile's `ends` row
static constexpr int kApBatch = 8;                              // samples per lane staged through LDS at a time
static constexpr int kApPitch = kApBatch + 1;                   // (double2 units)
static constexpr int kApSpeakAt = 2, kApPeakAt = 2 + kApCascade;    // offsets of the cascades in a component's state

enum : int { AP_CBL = 1, AP_SPEAK = 2, AP_MPEAK = 4, AP_PEAK0 = 8 };   // AP_PEAK0 << p: peak p steps (enabled and p < npeaks)

struct ApBiquad { double a0, a1, a2, b1, b2, fgain; };
struct ApParam { ApBiquad sp, pk[kApPeaks]; double mtau; int flags, pad; };

// xspeak's inner loop (iir.c:275-288) for one component: the input scaled by fgain, then kApStages direct-form-I biquads of one design
__host__ __device__ inline double ap_cascade(const ApBiquad &c, double *st, double x)
{
    double in = c.fgain * x;
    double p1 = st[0], p2 = st[1];
    st[0] = in; st[1] = p1;
#pragma unroll
    for (int n = 0; n < kApStages; n++) {
        const double o1 = st[2 + 2 * n], o2 = st[3 + 2 * n];
        const double y = c.a0 * in + c.a1 * p1 + c.a2 * p2 + c.b1 * o1 + c.b2 * o2;
        st[2 + 2 * n] = y; st[3 + 2 * n] = o1;
        p1 = o1; p2 = o2; in = y;
    }
    return in;
}

// one sample of one component through the stages that run, without xcbl's flush: what the host builds the carry matrices with
__host__ __device__ inline double ap_step_linear(const ApParam &q, double *s, double x)
{
    if (q.flags & AP_CBL) {
        const double y = x - s[0] + q.mtau * s[1];
        s[0] = x; s[1] = y;
        x = y;
    }
    if (q.flags & AP_SPEAK) x = ap_cascade(q.sp, s + kApSpeakAt, x);
    if (q.flags & AP_MPEAK) {
        double mix = 0.0;
#pragma unroll
        for (int p = 0; p < kApPeaks; p++)
            if (q.flags & (AP_PEAK0 << p)) mix += ap_cascade(q.pk[p], s + kApPeakAt + kApCascade * p, x);
        x = mix;
    }
    return x;
}

// both components of one sample through xcbl (with its |y| < 1e-100 -> 0, cblock.c:88-89), xspeak and xmpeak (the sum of the
// enabled peaks, exact zeros without any: iir.c:445-455); each stage for I and Q in one block, so the two chains interleave
__device__ __forceinline__ void ap_step2(const ApParam &q, double *s, double2 &v)
{
    double x = v.x, y = v.y;
    double *sq = s + kApDim;
    if (q.flags & AP_CBL) {
        const double ox = x - s[0] + q.mtau * s[1], oy = y - sq[0] + q.mtau * sq[1];
        s[0] = x; sq[0] = y;
        s[1] = fabs(ox) < 1.0e-100 ? 0.0 : ox;
        sq[1] = fabs(oy) < 1.0e-100 ? 0.0 : oy;
        x = ox; y = oy;
    }
    if (q.flags & AP_SPEAK) { x = ap_cascade(q.sp, s + kApSpeakAt, x); y = ap_cascade(q.sp, sq + kApSpeakAt, y); }
    if (q.flags & AP_MPEAK) {
        double mx = 0.0, my = 0.0;
#pragma unroll
        for (int p = 0; p < kApPeaks; p++)
            if (q.flags & (AP_PEAK0 << p)) {
                mx += ap_cascade(q.pk[p], s + kApPeakAt + kApCascade * p, x);
                my += ap_cascade(q.pk[p], sq + kApPeakAt + kApCascade * p, y);
            }
        x = mx; y = my;
    }
    v.x = x; v.y = y;
}

// Pass 0 / pass 1 (above).  One wavefront = 64 consecutive tiles of one channel; lane l owns samples [q L, min((q + 1) L, n)),
// q = 64 blockIdx.x + l.  kApBatch samples of every lane's tile travel HBM -> LDS with coalesced loads (runs of kApBatch samples
// per tile) and lane l takes row l out; pass 1's results leave the same way.  ends: [ch][estride], row q = kApW doubles.
template <int PASS>
static __global__ __launch_bounds__(64) void audio_peak_pass_kernel(double2 *buf, long long stride, int n, const int *list,
                                                                    const ApParam *prm, double *state, double *ends, long long estride, int L)
{
    __shared__ double2 lds[64 * kApPitch];
    const int ch = list[blockIdx.y], lane = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * 64;                    // first tile of this wavefront
    const long long first = t0 * L;
    if (first >= n) return;
    const long long ntile = ((long long)n + L - 1) / L;
    const long long q = t0 + lane;
    const bool live = PASS == 0 ? q < ntile - 1 : q < ntile;
    const ApParam p = prm[ch];
    double *erow = ends + (long long)ch * estride + q * kApW;
    double s[kApW];
#pragma unroll
    for (int i = 0; i < kApW; i++) s[i] = 0.0;
    if (PASS == 1 && live) {
#pragma unroll
        for (int i = 0; i < kApW; i++) s[i] = erow[i];
        if (p.flags & AP_CBL) {
            if (fabs(s[1]) < 1.0e-100) s[1] = 0.0;
            if (fabs(s[kApDim + 1]) < 1.0e-100) s[kApDim + 1] = 0.0;
        }
    }
    const long long tn = live ? ((long long)n - q * L < L ? (long long)n - q * L : (long long)L) : 0;     // samples of this lane's tile
    double2 *b = buf + (long long)ch * stride + first;
    const long long nrem = (long long)n - first;
    constexpr int B = kApBatch, RPI = 64 / B;
    const int frow = lane / B, fcol = lane % B;
    for (int i0 = 0; i0 < L; i0 += B) {
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int row = RPI * j + frow;
            const long long off = (long long)row * L + i0 + fcol;
            lds[row * kApPitch + fcol] = off < nrem ? b[off] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        double2 t[B];
#pragma unroll
        for (int k = 0; k < B; k++) t[k] = lds[lane * kApPitch + k];
        if (i0 + B <= tn) {
#pragma unroll
            for (int k = 0; k < B; k++) ap_step2(p, s, t[k]);
        } else if (i0 < tn) {
#pragma unroll
            for (int k = 0; k < B; k++)
                if (i0 + k < tn) ap_step2(p, s, t[k]);
        }
        if (PASS == 1) {
#pragma unroll
            for (int k = 0; k < B; k++) lds[lane * kApPitch + k] = t[k];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < B; j++) {
                const int row = RPI * j + frow;
                const long long off = (long long)row * L + i0 + fcol;
                if (off < nrem) b[off] = lds[row * kApPitch + fcol];
            }
        }
        __syncthreads();
    }
    if (PASS == 0 && live) {
#pragma unroll
        for (int i = 0; i < kApW; i++) erow[i] = s[i];
    }
    if (PASS == 1 && live && q == ntile - 1) {
        double *st = state + (long long)ch * kApW;
#pragma unroll
        for (int i = 0; i < kApW; i++) st[i] = s[i];
    }
}

// The carry, one wavefront per listed channel: lane r holds row r % kApDim of T (the same for I and Q) and element r of the state
// (component r / kApDim).  Row j of `ends` holds e_j (pass 0) and receives tile j's start state.
static __global__ __launch_bounds__(64) void audio_peak_carry_kernel(int n, int L, const int *list, const double *M, const double *state,
                                                                     double *ends, long long estride)
{
    __shared__ double sv[kApW];
    const int ch = list[blockIdx.x], lane = threadIdx.x, r = lane % kApDim, base = lane - r;
    const long long ntile = ((long long)n + L - 1) / L;
    double m[kApDim];
    const double *mr = M + ((long long)ch * kApDim + r) * kApDim;
#pragma unroll
    for (int k = 0; k < kApDim; k++) m[k] = mr[k];
    double s = state[(long long)ch * kApW + lane];
    double *e = ends + (long long)ch * estride + lane;
    double en = ntile > 1 ? e[0] : 0.0;
    for (long long j = 0; j < ntile; j++) {
        const double ej = en;
        if (j + 1 < ntile - 1) en = e[(j + 1) * kApW];              // the next tile's e, ahead of its use
        e[j * kApW] = s;
        if (j == ntile - 1) break;
        sv[lane] = s;
        __syncthreads();
        double a0 = ej, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (int k = 0; k < kApDim; k += 4) {
            a0 = fma(m[k], sv[base + k], a0);
            a1 = fma(m[k + 1], sv[base + k + 1], a1);
            a2 = fma(m[k + 2], sv[base + k + 2], a2);
            a3 = fma(m[k + 3], sv[base + k + 3], a3);
        }
        __syncthreads();
        s = (a0 + a1) + (a2 + a3);
    }
}

}  // namespace qh
