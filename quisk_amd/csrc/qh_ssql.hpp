// qh_ssql.hpp -- xssql of xrxa (wdsp/RXA.c:594, wdsp/ssql.c): the syllabic squelch, per listed channel, in place on the engine's rows
// at dsp rate, state carried from call to call.
//
// The detector is a chain of per-sample steps on the I component: a carrier block (cblock.c:74-94), a zero-crossing counter over the
// last kSsRing samples (xftov, ssql.c:70-108), a biquad low-pass (xdbqlp, iir.c:880-905), a window detector and a trigger
// (ssql.c:241-260); a four-state machine (ssql.c:262-296) turns the trigger into a real gain applied to I and Q.  Every step but the
// machine is a linear recurrence or a decision right behind one, so the call is cut into time tiles of L samples (L a multiple of 64),
// one tile per lane, and each recurrence gets its start values from a carry over the tiles, as qh_audio_peak.hpp does:
//   cbl 0    every tile but the last runs the blocker from zero and leaves its end state            (one read of the rows)
//   carry    (xp, y) <- Tc (xp, y) + e_j: every tile's blocker start
//   cbl 1    the blocker from the true start; the crossing bits, 64 samples a word                     (one read of the rows)
//   lp 0     windowed crossing counts (popcounts, then +in -out per sample) -> ftov -> biquad + window average from zero: end states
//   carry    (y1, y2, w) <- Tl (y1, y2, w) + e_j
//   lp 1     the same from the true start: the window detector's bits, and each tile's trigger map v -> alpha v + beta
//   carry    v <- alpha_j v + beta_j
//   trigger  the trigger from the true start: the trigger bits
//   walk     one wavefront per channel jumps from event to event (a trigger edge, a ramp's end) with __ballot over 64 words and
//            leaves the machine's (state, count) at every word's first sample; it also keeps the last kSsHist crossing bits
//   apply    every sample's gain from its word's (state, count) and trigger bits, I and Q times the gain     (one read, one write)
// Inside a tile the reference's recurrences are stepped as written (no contraction into FMAs); a carry only supplies start values.
// The blocker's 1e-100 flush is literal inside a tile and is applied to a carried output at a tile start (the carry itself is linear).
// The ramps are longer than a word (ntup, ntdown >= 64, checked by the engine), so a word holds at most two state changes and the apply
// pass finds them with two bit scans.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace qh {

static constexpr int kSsRing = 2400;                    // the ftov ring (RXA.c:459)
static constexpr int kSsHistW = 38;                     // words of crossing history kept per channel: 2432 >= kSsRing samples
static constexpr int kSsHist = 64 * kSsHistW;
static constexpr int kSsE = 4;                          // doubles per tile in `ends`
static constexpr int kSsBatch = 8, kSsPitch = kSsBatch + 1;
static constexpr double kSsTrThresh = 0.8197, kSsTrMute = 1.0, kSsTrUnmute = 0.3125;      // RXA.c:457, ssql.c:190-191
static constexpr double kSsEps = 0.01;                  // create_ftov, ssql.c:45

enum : int { SS_MUTED, SS_INCREASE, SS_UNMUTED, SS_DECREASE };

struct SsqlParam {
    double mtau;                        // dcbl (tau 0.02)
    double div;                         // ftov: fmax 2 rsize / rate
    double a0, a1, a2, b1, b2;          // dbqlp, fc 11.3, Q 1, gain 1, one stage
    double wdmult, wthresh;             // window detector
    double mute_mult, unmute_mult;      // trigger
    double muted_gain;
    double Tc[4], Tl[9];                // the blocker's and the low-pass + window's transitions over one tile with zero input
    int ntup, ntdown;
};

// Device state of one channel.  hist: bit k of word j is the crossing bit of the sample kSsHist - 64 j - k before the call's first
// (oldest first); in a call's crossing-bit row (xb) the same words come first, so sample i sits at bit i + kSsHist of the row.
struct SsqlState {
    double xp, y;                       // the blocker's last input and last output before its flush (= ftov's inlast)
    double y1, y2, w;                   // dbqlp's outputs, the window average
    double v;                           // the trigger voltage
    int state, count;
    unsigned long long hist[kSsHistW];
};

__device__ __forceinline__ double ss_ftov(int count, double div)
{
    const double r = (double)count / div;
    return 1.0 < r ? 1.0 : r;                           // min (1.0, rcount / div)
}

// bit k of the result: word sample ws + k lies in [lo, hi)
__device__ __forceinline__ unsigned long long ss_range(long long ws, long long lo, long long hi)
{
    long long a = lo - ws, b = hi - ws;
    a = a < 0 ? 0 : a > 64 ? 64 : a;
    b = b < 0 ? 0 : b > 64 ? 64 : b;
    if (a >= b) return 0ull;
    const unsigned long long top = b == 64 ? ~0ull : (1ull << b) - 1ull;
    return top & ~((1ull << a) - 1ull);
}

// the first set bit of `bits` at or after `from`, 64 if none
__device__ __forceinline__ int ss_first(unsigned long long bits, int from)
{
    const unsigned long long m = from >= 64 ? 0ull : bits & (~0ull << from);
    return m ? __ffsll((long long)m) - 1 : 64;
}

// cbl 0 / cbl 1.  One wavefront = 64 consecutive tiles of one channel; lane l owns samples [q L, min((q + 1) L, n)), q = 64 blockIdx.x
// + l; the I components travel HBM -> LDS in runs of kSsBatch samples per tile, coalesced.  ends: [ch][estride], row q = kSsE doubles.
template <int PASS>
static __global__ __launch_bounds__(64) void ssql_cbl_kernel(const double2 *buf, long long stride, int n, const int *list, const SsqlParam *prm,
                                                             SsqlState *state, double *ends, long long estride, unsigned long long *xb,
                                                             long long wstride, int L)
{
#pragma clang fp contract(off)
    __shared__ double lds[64 * kSsPitch];
    const int ch = list[blockIdx.y], lane = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * 64, first = t0 * L;
    if (first >= n) return;
    const long long ntile = ((long long)n + L - 1) / L, q = t0 + lane;
    const bool live = PASS == 0 ? q < ntile - 1 : q < ntile;
    const double mtau = prm[ch].mtau;
    double *erow = ends + (long long)ch * estride + q * kSsE;
    unsigned long long *xrow = xb + (long long)ch * wstride;
    if (PASS == 1 && blockIdx.x == 0 && lane < kSsHistW) xrow[lane] = state[ch].hist[lane];
    double xp = 0.0, yl = 0.0;                          // the last input; the last output as computed (the crossing test's)
    if (PASS == 1 && live) { xp = erow[0]; yl = erow[1]; }
    double yf = fabs(yl) < 1.0e-100 ? 0.0 : yl;         // ... and as the blocker keeps it
    const long long tn = live ? ((long long)n - q * L < L ? (long long)n - q * L : (long long)L) : 0;
    const double2 *b = buf + (long long)ch * stride + first;
    const long long nrem = (long long)n - first;
    unsigned long long *wout = xrow + kSsHistW + q * (L / 64), word = 0;
    constexpr int B = kSsBatch, RPI = 64 / B;
    const int frow = lane / B, fcol = lane % B;
    for (int i0 = 0; i0 < L; i0 += B) {
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int row = RPI * j + frow;
            const long long off = (long long)row * L + i0 + fcol;
            lds[row * kSsPitch + fcol] = off < nrem ? b[off].x : 0.0;
        }
        __syncthreads();
        if (i0 < tn) {
#pragma unroll
            for (int k = 0; k < B; k++) {
                if (i0 + k < tn) {
                    const double x = lds[lane * kSsPitch + k];
                    const double o = x - xp + mtau * yf;                       // cblock.c:84
                    if (PASS == 1 && yl * o < 0.0 && fabs(yl - o) > kSsEps) word |= 1ull << ((i0 + k) & 63);     // ssql.c:96-97
                    xp = x; yl = o;
                    yf = fabs(o) < 1.0e-100 ? 0.0 : o;                          // cblock.c:88
                }
            }
        }
        if (PASS == 1 && ((i0 + B) & 63) == 0) {
            if (i0 + B - 64 < tn) wout[(i0 + B - 64) >> 6] = word;
            word = 0;
        }
        __syncthreads();
    }
    if (PASS == 0 && live) { erow[0] = xp; erow[1] = yl; }
    if (PASS == 1 && live && q == ntile - 1) { state[ch].xp = xp; state[ch].y = yl; }
}

// A carry, one wavefront per listed channel: 64 tiles' rows at a time through LDS, lane 0 chains them (D <= 3 values, a few FMAs a
// tile).  Row j holds e_j (or, TRIG, the trigger map alpha_j, beta_j) and receives tile j's start state.  D = 2: the blocker (xp, y);
// D = 3: the low-pass and window (y1, y2, w); TRIG: the trigger voltage.
template <int D, bool TRIG>
static __global__ __launch_bounds__(64) void ssql_carry_kernel(int n, int L, const int *list, const SsqlParam *prm, const SsqlState *state,
                                                               double *ends, long long estride)
{
    __shared__ double e[64 * kSsE];
    const int ch = list[blockIdx.x], lane = threadIdx.x;
    const long long ntile = ((long long)n + L - 1) / L;
    const SsqlState &st = state[ch];
    const SsqlParam &p = prm[ch];
    double s[3], M[9];
    if (TRIG) s[0] = st.v;
    else if (D == 2) { s[0] = st.xp; s[1] = st.y; }
    else { s[0] = st.y1; s[1] = st.y2; s[2] = st.w; }
#pragma unroll
    for (int i = 0; i < D * D; i++) M[i] = D == 2 ? p.Tc[i] : p.Tl[i];
    double *rows = ends + (long long)ch * estride;
    for (long long j0 = 0; j0 < ntile; j0 += 64) {
        const int cnt = ntile - j0 < 64 ? (int)(ntile - j0) : 64;
        if (lane < cnt) {
#pragma unroll
            for (int k = 0; k < kSsE; k++) e[lane * kSsE + k] = rows[(j0 + lane) * kSsE + k];
        }
        __syncthreads();
        if (lane == 0) {
            for (int j = 0; j < cnt; j++) {
                double *r = e + j * kSsE;
                if (TRIG) {
                    const double a = r[0], c = r[1];
                    r[0] = s[0];
                    s[0] = a * s[0] + c;
                } else {
                    double nx[D];
#pragma unroll
                    for (int i = 0; i < D; i++) {
                        double acc = r[i];
#pragma unroll
                        for (int k = 0; k < D; k++) acc = fma(M[i * D + k], s[k], acc);
                        nx[i] = acc;
                    }
#pragma unroll
                    for (int i = 0; i < D; i++) { r[i] = s[i]; s[i] = nx[i]; }
                }
            }
        }
        __syncthreads();
        if (lane < cnt) {
#pragma unroll
            for (int k = 0; k < D; k++) rows[(j0 + lane) * kSsE + k] = e[lane * kSsE + k];
        }
        __syncthreads();
    }
}

// lp 0 / lp 1, one lane per tile (bits only).  The count of crossings in the kSsRing samples ending at the tile's sample -1 comes from
// popcounts of the row; from there each sample adds its own bit and drops the one kSsRing samples back (xftov's ring).  ftov at the
// tile's samples -1 and -2 are the biquad's x1, x2.  Pass 1 reads (y1, y2, w) from its row, then leaves the trigger map there.
template <int PASS>
static __global__ __launch_bounds__(64) void ssql_lp_kernel(int n, const int *list, const SsqlParam *prm, SsqlState *state, double *ends,
                                                            long long estride, const unsigned long long *xb, unsigned long long *wdb,
                                                            long long wstride, int L)
{
#pragma clang fp contract(off)
    const int ch = list[blockIdx.y];
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x, ntile = ((long long)n + L - 1) / L;
    if (PASS == 0 ? q >= ntile - 1 : q >= ntile) return;
    const SsqlParam &p = prm[ch];
    const double div = p.div, a0 = p.a0, a1 = p.a1, a2 = p.a2, b1 = p.b1, b2 = p.b2, wdmult = p.wdmult, wth = p.wthresh;
    const double mm = p.mute_mult, um = p.unmute_mult;
    const long long i0 = q * L, w0 = i0 >> 6;
    const int tn = (long long)n - i0 < L ? (int)((long long)n - i0) : L;
    const unsigned long long *x = xb + (long long)ch * wstride;
    int cnt = __popcll(x[w0] >> 32);                    // the samples i0 - 2400 .. i0 - 1: row bits i0 + 32 .. i0 + 2431
    for (int k = 1; k < kSsHistW; k++) cnt += __popcll(x[w0 + k]);
    const int cnt2 = cnt - (int)(x[w0 + kSsHistW - 1] >> 63) + (int)((x[w0] >> 31) & 1);     // ... i0 - 2401 .. i0 - 2
    double x1 = ss_ftov(cnt, div), x2 = ss_ftov(cnt2, div);
    double *erow = ends + (long long)ch * estride + q * kSsE;
    double y1 = 0.0, y2 = 0.0, w = 0.0;
    if (PASS == 1) { y1 = erow[0]; y2 = erow[1]; w = erow[2]; }
    double va = 0.0, alpha = 1.0;
    const double onem = 1.0 - wdmult;
    for (int b0 = 0; b0 < tn; b0 += 64) {
        const long long ws = (i0 + b0) >> 6;
        const unsigned long long in = x[kSsHistW + ws], out = (x[ws] >> 32) | (x[ws + 1] << 32);
        const int m = tn - b0 < 64 ? tn - b0 : 64;
        unsigned long long wbits = 0;
        for (int k = 0; k < m; k++) {
            cnt += (int)((in >> k) & 1) - (int)((out >> k) & 1);
            const double x0 = ss_ftov(cnt, div);
            const double y0 = a0 * x0 + a1 * x1 + a2 * x2 + b1 * y1 + b2 * y2;       // iir.c:890-895 (gain 1)
            y2 = y1; y1 = y0; x2 = x1; x1 = x0;
            w = wdmult * w + onem * y0;                                           // ssql.c:245
            if (PASS == 1) {
                const bool open = (y0 - w) > wth || (w - y0) > wth;                 // ssql.c:246-249: wd = 0
                wbits |= (unsigned long long)(open ? 0 : 1) << k;
                if (open) { va += (kSsTrUnmute - va) * um; alpha *= 1.0 - um; }
                else { va += (kSsTrMute - va) * mm; alpha *= 1.0 - mm; }
            }
        }
        if (PASS == 1) wdb[(long long)ch * wstride + ws] = wbits;
    }
    if (PASS == 0) { erow[0] = y1; erow[1] = y2; erow[2] = w; }
    else {
        erow[0] = alpha; erow[1] = va;
        if (q == ntile - 1) { state[ch].y1 = y1; state[ch].y2 = y2; state[ch].w = w; }
    }
}

// the trigger (ssql.c:252-260) from each tile's true start voltage: the trigger bits (1 = open)
static __global__ __launch_bounds__(64) void ssql_trigger_kernel(int n, const int *list, const SsqlParam *prm, SsqlState *state,
                                                                 const double *ends, long long estride, const unsigned long long *wdb,
                                                                 unsigned long long *trb, long long wstride, int L)
{
#pragma clang fp contract(off)
    const int ch = list[blockIdx.y];
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x, ntile = ((long long)n + L - 1) / L;
    if (q >= ntile) return;
    const double mm = prm[ch].mute_mult, um = prm[ch].unmute_mult;
    const long long i0 = q * L;
    const int tn = (long long)n - i0 < L ? (int)((long long)n - i0) : L;
    double v = ends[(long long)ch * estride + q * kSsE];
    const unsigned long long *wd = wdb + (long long)ch * wstride;
    unsigned long long *tr = trb + (long long)ch * wstride;
    for (int b0 = 0; b0 < tn; b0 += 64) {
        const long long ws = (i0 + b0) >> 6;
        const unsigned long long wb = wd[ws];
        const int m = tn - b0 < 64 ? tn - b0 : 64;
        unsigned long long tb = 0;
        for (int k = 0; k < m; k++) {
            if ((wb >> k) & 1) v += (kSsTrMute - v) * mm;
            else v += (kSsTrUnmute - v) * um;
            tb |= (unsigned long long)(v > kSsTrThresh ? 0 : 1) << k;
        }
        tr[ws] = tb;
    }
    if (q == ntile - 1) state[ch].v = v;
}

// The event walk, one wavefront per listed channel.  64 words (4096 samples) at a time, lane l holding word l's trigger bits: while
// MUTED / UNMUTED the next set / clear bit is found with one __ballot and a bit scan, a ramp is skipped whole.  rec[w] = state | count
// << 2 at word w's first sample.  Then the channel's (state, count) and the last kSsHist crossing bits go to its state.
static __global__ __launch_bounds__(64) void ssql_walk_kernel(int n, const int *list, const SsqlParam *prm, SsqlState *state,
                                                              const unsigned long long *trb, int *rec, const unsigned long long *xb, long long wstride)
{
    const int ch = list[blockIdx.x], lane = threadIdx.x;
    const int ntup = prm[ch].ntup, ntdown = prm[ch].ntdown;
    SsqlState *st = state + ch;
    int S = st->state, c = st->count;
    const unsigned long long *t = trb + (long long)ch * wstride;
    int *r = rec + (long long)ch * wstride;
    const long long nw = ((long long)n + 63) / 64;
    for (long long c0 = 0; c0 < nw; c0 += 64) {
        const long long wi = c0 + lane, ws = wi * 64, cs = c0 * 64, ce = cs + 4096 < n ? cs + 4096 : n;
        const unsigned long long tw = wi < nw ? t[wi] : 0ull;
        int mine = 0;
        long long pp = cs;
        while (pp < ce) {
            if (S == SS_MUTED || S == SS_UNMUTED) {
                const unsigned long long m = (S == SS_MUTED ? tw : ~tw) & ss_range(ws, pp, ce);
                const unsigned long long bal = __ballot(m != 0ull);
                long long hit = ce;
                if (bal) {
                    const int l0 = __ffsll((long long)bal) - 1;
                    const unsigned long long ml = __shfl(m, l0);
                    hit = (c0 + l0) * 64 + __ffsll((long long)ml) - 1;
                }
                if (ws >= pp && ws <= hit && ws < ce) mine = S;
                if (hit >= ce) break;
                S = S == SS_MUTED ? SS_INCREASE : SS_DECREASE;      // ssql.c:267-272, :281-286
                c = S == SS_INCREASE ? ntup : ntdown;
                pp = hit + 1;
            } else {
                const long long last = pp + c;                       // the ramp's last sample (count 0)
                if (ws >= pp && ws <= last && ws < ce) mine = S | ((c - (int)(ws - pp)) << 2);
                if (last < ce) { S = S == SS_INCREASE ? SS_UNMUTED : SS_MUTED; c = -1; pp = last + 1; }
                else { c -= (int)(ce - pp); pp = ce; }
            }
        }
        if (wi < nw) r[wi] = mine;
    }
    if (lane < kSsHistW) {                                           // row bits n .. n + kSsHist - 1
        const unsigned long long *x = xb + (long long)ch * wstride;
        const long long a = ((long long)n >> 6) + lane;
        const int sh = n & 63;
        st->hist[lane] = sh ? (x[a] >> sh) | (x[a + 1] << (64 - sh)) : x[a];
    }
    if (lane == 0) { st->state = S; st->count = c; }
}

// The gain of every sample from its word's (state, count) and trigger bits, I and Q multiplied in place (also by 0: a NaN stays).
// With ramps longer than a word: MUTED -> muted up to the first set bit t, then cup[k - t - 1]; UNMUTED -> 1 up to the first clear
// bit u, then cdown[k - u - 1]; a ramp with count c runs to k = c and continues as the state after it.
static __global__ __launch_bounds__(256) void ssql_apply_kernel(double2 *buf, long long stride, int n, const int *list, const SsqlParam *prm,
                                                                const unsigned long long *trb, const int *rec, long long wstride,
                                                                const double *cup, const double *cdown)
{
    const int ch = list[blockIdx.y];
    const int ntup = prm[ch].ntup, ntdown = prm[ch].ntdown;
    const double mg = prm[ch].muted_gain;
    const unsigned long long *t = trb + (long long)ch * wstride;
    const int *r = rec + (long long)ch * wstride;
    double2 *row = buf + (long long)ch * stride;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long wi = i >> 6;
        const int k = (int)(i & 63), rv = r[wi], S = rv & 3, c = rv >> 2;
        const unsigned long long tb = t[wi];
        double g;
        if (S == SS_INCREASE && k <= c) g = cup[ntup - c + k];
        else if (S == SS_DECREASE && k <= c) g = cdown[ntdown - c + k];
        else if (S == SS_MUTED || S == SS_DECREASE) {
            const int f = ss_first(tb, S == SS_MUTED ? 0 : c + 1);
            g = k <= f ? mg : cup[k - f - 1];
        } else {
            const int f = ss_first(~tb, S == SS_UNMUTED ? 0 : c + 1);
            g = k <= f ? 1.0 : cdown[k - f - 1];
        }
        double2 z = row[i];
        z.x = z.x * g; z.y = z.y * g;
        row[i] = z;
    }
}

// flush_ssql (ssql.c:208-220): the blocker, the ftov ring and inlast, the biquad; not the window average, the trigger or the machine
static __global__ __launch_bounds__(64) void ssql_flush_kernel(SsqlState *state)
{
    SsqlState &st = state[blockIdx.x];
    const int lane = threadIdx.x;
    if (lane == 0) { st.xp = 0.0; st.y = 0.0; st.y1 = 0.0; st.y2 = 0.0; }
    if (lane < kSsHistW) st.hist[lane] = 0ull;
}

}  // namespace qh
