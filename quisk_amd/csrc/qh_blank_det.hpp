// qh_blank_det.hpp -- the impulse detector WDSP's two noise blankers share (xanb, wdsp/nob.c:118-122; xnob, wdsp/nobII.c:179-184), for
// the banks of qh_anb.hip and qh_nob.hip.
//
// The reference steps, per sample: mag = |x|; avg = backmult avg + (1 - backmult) mag; the sample is flagged when mag > avg threshold.
// avg is a linear recurrence, so a call is cut as qh_ssql.hpp cuts the syllabic squelch, into time tiles of kDetL samples, one per lane:
//   det 0    avg stepped from 0 over every tile but the last, each tile's end value                                (one read of the rows)
//   carry    a <- backmult^L a + e_j over the tiles (an affine scan, 64 tiles a step): every tile's true start value
//   det 1    avg from the true start, the reference's two multiplies and one add in its order, uncontracted; the flags, 64 samples
//            a word, and the channel's avg behind the call                                                         (one read of the rows)
// avg inside a tile is the reference's recurrence; only its start value carries the rounding of the scan, eps / (1 - backmult) relative
// at worst, so a flag can differ from a sample-serial run only where mag sits that close to avg threshold.
//
// The kernels are templates over a bank's parameter and state structs: Param has backmult, ombackmult, threshold, carry (backmult^kDetL)
// and run, State has avg; each bank keeps its own layout and uploads nothing twice.
#pragma once
#include <climits>
#include "qh_bank.hpp"

namespace qh {

typedef unsigned long long u64;

constexpr int kDetL = 128;                              // samples per lane tile (two words of flags)
constexpr int kDetB = 8, kDetPitch = kDetB + 1;         // samples per tile and trip through LDS; padded against bank conflicts

// every set bit smeared over the T - 1 bits above it (inside the word)
__device__ __forceinline__ u64 dilate(u64 x, int T)
{
    if (!x) return 0ull;
    if (T >= 64) return ~0ull << (__ffsll((long long)x) - 1);
    u64 r = x;
    for (int have = 1; have < T;) {
        const int sh = have < T - have ? have : T - have;
        r |= r << sh;
        have += sh;
    }
    return r;
}

// det 0 / det 1.  One wavefront = 64 consecutive tiles of one channel; lane l owns samples [q L, min((q + 1) L, n)), q = 64 blockIdx.x
// + l.  The samples travel HBM -> |x| -> LDS in runs of kDetB per tile (128 contiguous bytes per eight lanes), each lane then steps
// its own row.  ends: [ch][estride], one double per tile.  trb: [ch][wstride] words of flags, bits at and beyond n clear in the words
// written (words wholly beyond n are not written).
template <int PASS, typename Param, typename State>
__global__ __launch_bounds__(64) void det_kernel(const double2 *in, long long stride, int n, const Param *prm, State *state, double *ends,
                                                 long long estride, u64 *trb, long long wstride)
{
#pragma clang fp contract(off)
    constexpr int L = kDetL, B = kDetB, RPI = 64 / B;
    __shared__ double lds[64 * kDetPitch];
    const int ch = blockIdx.y, lane = threadIdx.x;
    if (!prm[ch].run) return;
    const long long t0 = (long long)blockIdx.x * 64, first = t0 * L;
    const long long ntile = ((long long)n + L - 1) / L, q = t0 + lane;
    if (first >= n || (PASS == 0 && t0 >= ntile - 1)) return;
    const bool live = PASS == 0 ? q < ntile - 1 : q < ntile;
    const double bm = prm[ch].backmult, om = prm[ch].ombackmult, th = prm[ch].threshold;
    double *erow = ends + (long long)ch * estride;
    double avg = PASS == 1 && live ? erow[q] : 0.0;
    const int tn = live ? (int)((long long)n - q * L < L ? (long long)n - q * L : (long long)L) : 0;
    const double2 *b = in + (long long)ch * stride + first;
    const long long nrem = (long long)n - first;
    u64 *wout = trb + (long long)ch * wstride + q * (L / 64), word = 0;
    const int frow = lane / B, fcol = lane % B;
    for (int i0 = 0; i0 < L; i0 += B) {
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int row = RPI * j + frow;
            const long long off = (long long)row * L + i0 + fcol;
            double m = 0.0;
            if (off < nrem) {
                const double2 z = b[off];
                m = __builtin_sqrt(z.x * z.x + z.y * z.y);                  // nob.c:118, nobII.c:179
            }
            lds[row * kDetPitch + fcol] = m;
        }
        __syncthreads();
        if (i0 < tn) {
#pragma unroll
            for (int k = 0; k < B; k++) {
                if (i0 + k < tn) {
                    const double mag = lds[lane * kDetPitch + k];
                    avg = bm * avg + om * mag;                              // nob.c:119, nobII.c:180
                    if (PASS == 1 && mag > avg * th) word |= 1ull << ((i0 + k) & 63);      // nob.c:122, nobII.c:181
                }
            }
        }
        if (PASS == 1 && ((i0 + B) & 63) == 0) {
            if (i0 + B - 64 < tn) wout[(i0 + B - 64) >> 6] = word;
            word = 0;
        }
        __syncthreads();
    }
    if (PASS == 0 && live) erow[q] = avg;
    if (PASS == 1 && live && q == ntile - 1) state[ch].avg = avg;
}

// The carry, one wavefront per channel: 64 tiles a step, the maps a -> M a + e_j composed by a scan over the lanes.  Row j holds e_j
// (tiles before the last) and receives tile j's start value.  (Explicit fmas and one product: the same under any contraction setting.)
template <typename Param, typename State>
__global__ __launch_bounds__(64) void carry_kernel(int n, const Param *prm, const State *state, double *ends, long long estride)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    if (!prm[ch].run) return;
    const long long ntile = ((long long)n + kDetL - 1) / kDetL;
    const double M = prm[ch].carry;
    double s = state[ch].avg;
    double *rows = ends + (long long)ch * estride;
    for (long long j0 = 0; j0 < ntile; j0 += 64) {
        const long long j = j0 + lane;
        double A = M, E = j < ntile - 1 ? rows[j] : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double Au = __shfl_up(A, d, 64), Eu = __shfl_up(E, d, 64);
            if (lane >= d) { E = fma(A, Eu, E); A *= Au; }
        }
        const double Ax = __shfl_up(A, 1, 64), Ex = __shfl_up(E, 1, 64);
        if (j < ntile) rows[j] = lane ? fma(Ax, s, Ex) : s;
        s = fma(__shfl(A, 63, 64), s, __shfl(E, 63, 64));
    }
}

// det 0, the carry and det 1 of one call of n samples on the bank's stream; the flags are in h.d_trb (row stride h.nw) behind them.
template <typename Param, typename State>
void det_enqueue(const DetBank &h, const double2 *in, long long in_stride, int n, const Param *d_prm, State *d_state)
{
    const unsigned ntile = (unsigned)((n + kDetL - 1) / kDetL), nch = (unsigned)h.nch;
    if (ntile > 1)
        hipLaunchKernelGGL((det_kernel<0, Param, State>), dim3((ntile + 63) / 64, nch), dim3(64), 0, h.stream, in, in_stride, n, d_prm, d_state,
                           h.d_ends, h.nt, h.d_trb, h.nw);
    hipLaunchKernelGGL((carry_kernel<Param, State>), dim3(nch), dim3(64), 0, h.stream, n, d_prm, (const State *)d_state, h.d_ends, h.nt);
    hipLaunchKernelGGL((det_kernel<1, Param, State>), dim3((ntile + 63) / 64, nch), dim3(64), 0, h.stream, in, in_stride, n, d_prm, d_state,
                       h.d_ends, h.nt, h.d_trb, h.nw);
}

}  // namespace qh
