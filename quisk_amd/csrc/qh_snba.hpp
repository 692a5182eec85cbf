// qh_snba.hpp -- WDSP's SNBA (spectral noise blanker, wdsp/snb.c:31-577 with asolve / median / trI / dR of wdsp/lmath.c:29-186
// and the two polyphase resamplers of wdsp/resample.c:120-157) on gfx950.
//
// One wavefront per channel: the block is a chain of short, strictly ordered recurrences (an order-64 Levinson solve per
// 256-sample frame, a median, a run scanner, then per corrupt run another solve, a Toeplitz inverse and a banded
// least-squares interpolation), so the parallelism is the channels; inside a channel the 64 lanes take one output each of
// every sum that has independent outputs (autocorrelation lags, residue samples, polyphase outputs, matrix rows), each lane
// adding its terms in the reference's order, and the scalar recurrences run redundantly in all lanes from LDS broadcasts.
// Every sum therefore has the reference's operation order (fp contraction off), which keeps the threshold decisions of the
// detector identical.  The structured matrices A1 / A2 of xHat (snb.c:265-304) are never built: their entries are read off
// the predictor `a` while P1 = A1'A2 is formed; the Toeplitz inverse (up to xsize x xsize) lives in a per-channel scratch.
//
// Two forms.  The single kernel (snba_kernel<false>) keeps both polyphase resamplers inside the serial block loop with their
// windows in LDS: dsp_rate up to 48 kHz and dsp_size up to kSnbFusedMaxDsp.  The three-pass form takes them out, since they are
// plain FIRs with no feedback from the frames: snba_decim_kernel makes the 12 kHz row of every listed channel for the whole call,
// one thread per output; snba_kernel<true> runs the frames from that row into a second 12 kHz row, block by block with the same
// ring indices; snba_interp_kernel writes the channel's row at the DSP rate, one thread per output.  snba_hist_kernel leaves
// each resampler's history behind its pass.  Every sum has the same terms in the same order in both forms, so they agree in
// every bit.  The second form runs ratios up to 32 (dsp_rate 384 kHz) and dsp_size up to kSnbMaxDsp.
#pragma once
#include <hip/hip_runtime.h>
#include "qh_wave.hpp"

namespace qh {

constexpr int kSnbX = 256;          // xsize, RXA.c:245
constexpr int kSnbMaxImp = 256;     // MAXIMP, snb.c:29
constexpr int kSnbMaxDsp = 4096;    // dsp_size limit of the blanker (the three-pass form)
constexpr int kSnbMaxRatio = 32;    // dsp_rate / 12000 up to 384 kHz (cpp_in = 140 * ratio + 1; the state's off_rin holds cpp_in - 1 samples)
constexpr int kSnbFusedMaxDsp = 1024;       // the single kernel: dsp_size and ...
constexpr int kSnbFusedMaxRatio = 4;        // ... dsp_rate / 12000 its LDS windows are made for
constexpr int kSnbFusedMaxCppIn = 140 * kSnbFusedMaxRatio + 1;

struct SnbaParam {
    int ratio, isize, incr, iasize, oasize, init_oaoutidx, cpp_in, cpp_out;     // calc_snba, snb.c:31-66
    int asize, npasses, b, pre, post, pad;
    double k1, k2, pmultmin;
    // state layout (doubles per channel)
    int off_inacc, off_outacc, off_rin, off_rout, state_doubles, pad2;
};
struct SnbaIdx { int iainidx, iaoutidx, nsamps, oainidx, oaoutidx, pad[3]; };
// what the tuning setters change, per channel (SetRXASNBAasize / npasses / k1 / k2 / bridge / presamps / postsamps / pmultmin,
// snb.c:604-658); the defaults are create_rxa's (RXA.c:183-202)
struct SnbaTune { int asize, npasses, b, pre, post, pad; double k1, k2, pmultmin; };

struct SnbaLds {
    double xb[2 * kSnbX];           // xbase | xaux
    double savex[kSnbX], v[kSnbX], vpwr[kSnbX], a[kSnbX], r[kSnbX + 1], z[kSnbX + 1], p2[kSnbX], xout[kSnbX], y[kSnbX], vv[kSnbX];
    double merit[kSnbMaxImp];
    double scal[4];
    int det[kSnbX], unfixed[kSnbX], bimp[kSnbMaxImp], limp[kSnbMaxImp], bef[kSnbMaxImp + 1], aft[kSnbMaxImp], popt[kSnbMaxImp],
        nextl[kSnbMaxImp];
    int nimp, next;
};

// the single kernel's resampler windows; the three-pass form's frame kernel has none
template <bool ON> struct SnbaRsLds {
    double sin_[kSnbFusedMaxCppIn - 1 + kSnbFusedMaxDsp];   // input resampler: history | block (real parts)
    double sob[140 + kSnbFusedMaxDsp];                      // output resampler: history | 12 kHz block
};
template <> struct SnbaRsLds<false> { double sin_[1], sob[1]; };

// asolve, lmath.c:96-127: x has at least asize valid samples in front of it
static __device__ void snba_asolve(SnbaLds &s, int xsize, int asize, const double *x, int lane)
{
#pragma clang fp contract(off)
    {   // lags lane and lane + 64 side by side (asize <= 64: the second one is lag 64 in lane 0); each sum in the order j = 0 .. xsize - 1
        double acc = 0.0, acc2 = 0.0;
        const double *xa = x - lane, *xb2 = x - lane - 64;
#pragma unroll 8
        for (int j = 0; j < xsize; j++) {
            const double xj = x[j];
            acc += xj * xa[j];
            acc2 += xj * xb2[j];
        }
        if (lane <= asize) { s.r[lane] = acc; s.z[lane] = lane == 0 ? 1.0 : 0.0; }
        if (lane + 64 <= asize) { s.r[lane + 64] = acc2; s.z[lane + 64] = 0.0; }
    }
    __syncthreads();
    double beta = s.r[0];
    for (int k = 0; k < asize; k++) {
        // the products in parallel, their sum in the reference's order j = 0 .. k (one readlane + one subtract per term)
        const double prod = lane <= k ? s.z[lane] * s.r[k + 1 - lane] : 0.0;
        double alpha = 0.0;
        for (int j = 0; j <= k; j++) alpha -= lane_bcast(prod, j);
        alpha /= beta;
        const int half = (k + 1) / 2;
        double zi = 0.0, zo = 0.0;
        if (lane <= half) { zi = s.z[lane]; zo = s.z[k + 1 - lane]; }
        __syncthreads();
        if (lane <= half) {
            const double t = zo + alpha * zi;
            s.z[lane] = zi + alpha * zo;
            s.z[k + 1 - lane] = t;
        }
        __syncthreads();
        beta *= 1.0 - alpha * alpha;
    }
    for (int i = lane; i < asize; i += 64) {
        double t = -s.z[i + 1];
        if (t != t) t = 0.0;
        s.a[i] = t;
    }
    __syncthreads();
}

// invf, snb.c:306-322
static __device__ void snba_invf(SnbaLds &s, int xsize, int asize, const double *x, int lane)
{
#pragma clang fp contract(off)
    for (int i = lane; i < xsize; i += 64) {
        double acc = 0.0;
        if (i >= asize && i < xsize - asize) {
            for (int j = 0; j < asize; j++) acc += s.a[j] * (x[i - 1 - j] + x[i + 1 + j]);
            acc = x[i] - 0.5 * acc;
        } else if (i >= xsize - asize) {
            for (int j = 0; j < asize; j++) acc += s.a[j] * x[i - 1 - j];
            acc = x[i] - acc;
        }
        s.v[i] = acc;
    }
    __syncthreads();
}

// det, snb.c:324-402
static __device__ void snba_det(SnbaLds &s, const SnbaParam &q, int asize, int lane)
{
#pragma clang fp contract(off)
    const int xs = kSnbX, n = xs - asize, kth = n / 2;
    for (int i = lane; i < xs; i += 64) s.vpwr[i] = i >= asize ? s.v[i] * s.v[i] : 0.0;
    __syncthreads();
    // median (lmath.c:129-186 selects the element of rank n / 2): rank by counting
    for (int i = asize + lane; i < xs; i += 64) {
        const double e = s.vpwr[i];
        int rank = 0;
        for (int j = asize; j < xs; j++) {
            const double o = s.vpwr[j];
            rank += (o < e || (o == e && j < i)) ? 1 : 0;
        }
        if (rank == kth) s.scal[0] = e;
    }
    __syncthreads();
    const double t1 = q.k1 * s.scal[0];
    double t2 = 0.0;
    for (int base = asize; base < xs; base += 64) {        // contributions in parallel (0.0 where the reference adds nothing), summed in order
        const int i = base + lane;
        const double p = i < xs ? s.vpwr[i] : 0.0;
        double c = 0.0;
        if (i < xs) { if (p <= t1) c = p; else if (p <= 2.0 * t1) c = 2.0 * t1 - p; }
        const int cnt = xs - base < 64 ? xs - base : 64;
        for (int j = 0; j < cnt; j++) t2 += lane_bcast(c, j);
    }
    t2 *= q.k2 / (double)n;
    for (int i = lane; i < xs; i += 64) s.det[i] = (i >= asize && s.vpwr[i] > t2) ? 1 : 0;
    __syncthreads();
    if (lane == 0) {
        int bstate = 0, bcount = 0, bsamp = 0;
        for (int i = asize; i < xs; i++) {
            const int d = s.det[i];
            if (bstate == 0) { if (d == 1) bstate = 1; }
            else if (bstate == 1) { if (d == 0) { bstate = 2; bsamp = i; bcount = 1; } }
            else {
                ++bcount;
                if (bcount > q.b) bstate = d == 1 ? 1 : 0;
                else if (d == 1) {
                    for (int j = bsamp; j < bsamp + bcount - 1; j++) s.det[j] = 1;
                    bstate = 1;
                }
            }
        }
        for (int i = asize; i < xs; i++)
            if (s.det[i] == 1)
                for (int j = i - 1; j > i - 1 - q.pre; j--) if (j >= asize) s.det[j] = 1;
        for (int i = xs - 1; i >= asize; i--)
            if (s.det[i] == 1)
                for (int j = i + 1; j < i + 1 + q.post; j++) if (j < xs) s.det[j] = 1;
    }
    __syncthreads();
}

// scanFrame, snb.c:404-490 (lane 0; results in LDS)
static __device__ void snba_scan(SnbaLds &s, int xsize, int pval, double pmultmin, const int *det, int lane)
{
#pragma clang fp contract(off)
    if (lane == 0) {
        int inflag = 0, nimp = 0;
        for (int i = 0; i <= kSnbMaxImp; i++) s.bef[i] = 0;
        for (int i = 0; i < kSnbMaxImp; i++) s.aft[i] = 0;
        for (int i = 0; i < xsize && nimp < kSnbMaxImp; i++) {
            const int d = det[i];
            if (d == 1 && inflag == 0) { inflag = 1; s.bimp[nimp] = i; s.limp[nimp] = 1; nimp++; }
            else if (d == 1) s.limp[nimp - 1]++;
            else {
                inflag = 0;
                s.bef[nimp]++;
                if (nimp > 0) s.aft[nimp - 1]++;
            }
        }
        for (int i = 0; i < nimp; i++) {
            int p = s.bef[i] < s.aft[i] ? s.bef[i] : s.aft[i];
            if (p > pval) p = pval;
            if (p < (int)(pmultmin * s.limp[i])) p = -1;
            s.popt[i] = p;
            s.merit[i] = (double)p / (double)s.limp[i];
            s.nextl[i] = i;
        }
        for (int j = 0; j < nimp - 1; j++)
            for (int k = 0; k < nimp - j - 1; k++)
                if (s.merit[k] < s.merit[k + 1]) {
                    const double td = s.merit[k]; const int ti = s.nextl[k];
                    s.merit[k] = s.merit[k + 1]; s.nextl[k] = s.nextl[k + 1];
                    s.merit[k + 1] = td; s.nextl[k + 1] = ti;
                }
        int i = 1;
        if (nimp > 0) while (i < nimp && s.merit[i] == s.merit[0]) i++;
        for (int j = 0; j < i - 1; j++)
            for (int k = 0; k < i - j - 1; k++)
                if (s.limp[s.nextl[k]] < s.limp[s.nextl[k + 1]]) {
                    const double td = s.merit[k]; const int ti = s.nextl[k];
                    s.merit[k] = s.merit[k + 1]; s.nextl[k] = s.nextl[k + 1];
                    s.merit[k + 1] = td; s.nextl[k + 1] = ti;
                }
        s.nimp = nimp;
        s.next = nimp > 0 ? s.nextl[0] : 0;
    }
    __syncthreads();
}

// xHat, snb.c:265-304: the n = xusize unknown samples from p known ones either side (xk = first known sample)
static __device__ void snba_xhat(SnbaLds &s, int n, int p, const double *xk, double *B, int lane)
{
#pragma clang fp contract(off)
    const double *a = s.a;
    // ATAc0 (snb.c:209-216): r[i] = sum_j A1[j][i] A1[j][0]; column 0 of A1 is 1, -a[0], ..., -a[p-1]
    for (int i = lane; i < n; i += 64) {
        double acc = 0.0;
        for (int j = 0; j <= p; j++) {
            const double c0 = j == 0 ? 1.0 : -a[j - 1];
            double ci = 0.0;
            if (j == i) ci = 1.0;
            else if (j > i && j <= i + p) ci = -a[j - i - 1];
            acc += ci * c0;
        }
        s.r[i] = acc;
    }
    __syncthreads();
    // trI (lmath.c:52-94)
    const double scale = 1.0 / s.r[0];
    __syncthreads();
    for (int i = lane; i < n; i += 64) s.r[i] *= scale;
    for (int i = lane; i < n; i += 64) { s.y[i] = 0.0; s.vv[i] = 0.0; }
    __syncthreads();
    {   // dR (lmath.c:29-50) on n - 1 unknowns
        const int m = n - 1;
        if (lane == 0) s.y[0] = -s.r[1];
        __syncthreads();
        double alpha = -s.r[1], beta = 1.0;
        for (int k = 0; k < m - 1; k++) {
            beta *= 1.0 - alpha * alpha;
            double gamma = 0.0;
            for (int j = 0; j <= k; j++) gamma += s.r[k + 1 - j] * s.y[j];
            alpha = -(s.r[k + 2] + gamma) / beta;
            __syncthreads();
            for (int i = lane; i <= k; i += 64) s.z[i] = s.y[i] + alpha * s.y[k - i];
            __syncthreads();
            for (int i = lane; i <= k; i += 64) s.y[i] = s.z[i];
            if (lane == 0) s.y[k + 1] = alpha;
            __syncthreads();
        }
    }
    double t = 0.0;
    for (int i = 0; i < n - 1; i++) t += s.r[i + 1] * s.y[i];
    const double gamma = 1.0 / (1.0 + t);
    for (int i = lane; i < n - 1; i += 64) s.vv[i] = gamma * s.y[n - 2 - i];
    __syncthreads();
    for (int i = lane; i < n; i += 64) B[i] = i == 0 ? gamma : s.vv[n - 1 - i];
    __syncthreads();
    for (int i = 1; i <= (n - 1) / 2; i++) {
        for (int j = i + lane; j < n - i; j += 64)
            B[i * n + j] = B[(i - 1) * n + (j - 1)] + (s.vv[n - j - 1] * s.vv[n - i - 1] - s.vv[i - 1] * s.vv[j - 1]) / gamma;
        __syncthreads();
    }
    for (int i = 0; i <= (n - 1) / 2; i++)
        for (int j = i + lane; j < n - i; j += 64) {
            const double b = B[i * n + j] * scale;
            const int ni = n - i - 1, nj = n - j - 1;
            B[i * n + j] = b; B[j * n + i] = b; B[ni * n + nj] = b; B[nj * n + ni] = b;
        }
    // P2 = (A1'A2 restricted to the known columns) xk: multA1TA2 + multXKE, snb.c:218-252
    const int q2 = n + 2 * p;
    for (int i = lane; i < n; i += 64) {
        double acc = 0.0;
        for (int col = i; col < p; col++) {                 // known samples in front: A2[k][col] = a[p-1-col+k] for k <= col
            double e = 0.0;
            const int kmax = i + p < col ? i + p : col;
            for (int k = i; k <= kmax; k++) {
                const double a1 = k == i ? 1.0 : -a[k - i - 1];
                e += a1 * a[p - 1 - col + k];
            }
            acc += e * xk[col];
        }
        for (int col = q2 - p; col <= q2 - n + i; col++) {  // known samples behind: A2[c][col] = -1, A2[k][col] = a[k-c-1] below it, c = col - p
            double e = 0.0;
            const int c = col - p;
            for (int k = (i > c ? i : c); k <= i + p; k++) {
                const double a1 = k == i ? 1.0 : -a[k - i - 1];
                const double a2 = k == c ? -1.0 : a[k - c - 1];
                e += a1 * a2;
            }
            acc += e * xk[col];
        }
        s.p2[i] = acc;
    }
    __syncthreads();
    // multAv, snb.c:254-263 (B is symmetric: read the transposed element for coalescing)
    for (int i = lane; i < n; i += 64) {
        double acc = 0.0;
        for (int k = 0; k < n; k++) acc += B[k * n + i] * s.p2[k];
        s.xout[i] = acc;
    }
    __syncthreads();
}

// execFrame, snb.c:492-537; x = s.xb + xsize
static __device__ void snba_frame(SnbaLds &s, const SnbaParam &q, double *B, int lane)
{
#pragma clang fp contract(off)
    const int xs = kSnbX;
    double *x = s.xb + xs;
    for (int i = lane; i < xs; i += 64) s.savex[i] = x[i];
    __syncthreads();
    snba_asolve(s, xs, q.asize, x, lane);
    snba_invf(s, xs, q.asize, x, lane);
    snba_det(s, q, q.asize, lane);
    for (int i = lane; i < xs; i += 64) if (s.det[i] != 0) x[i] = 0.0;
    __syncthreads();
    snba_scan(s, xs, q.asize, q.pmultmin, s.det, lane);
    const int nimp = s.nimp;
    for (int pass = 0; pass < q.npasses; pass++) {
        for (int i = lane; i < xs; i += 64) s.unfixed[i] = s.det[i];
        __syncthreads();
        for (int k = 0; k < nimp; k++) {
            if (k > 0) snba_scan(s, xs, q.asize, q.pmultmin, s.unfixed, lane);
            const int next = s.next, p = s.popt[next], b0 = s.bimp[next], len = s.limp[next];
            __syncthreads();
            if (p > 0) {
                snba_asolve(s, xs, p, x, lane);
                snba_xhat(s, len, p, x + b0 - p, B, lane);
                for (int i = lane; i < len; i += 64) { x[b0 + i] = s.xout[i]; s.unfixed[b0 + i] = 0; }
            } else
                for (int i = lane; i < len; i += 64) x[b0 + i] = s.savex[b0 + i];
            __syncthreads();
        }
    }
}

// rows of the listed channels from one chain buffer to the other
static __global__ __launch_bounds__(NT) void copy_rows_kernel(const double2 *src, double2 *dst, long long stride, int n, const int *chan_list)
{
    const long long o = (long long)chan_list[blockIdx.y] * stride;
    for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) dst[o + i] = src[o + i];
}

// xsnba (snb.c:539-571) over nblk blocks of dsp_size samples, in place on the channel's row of buf.  ROWS: the three-pass form's
// frame kernel -- the two resamplers run in passes of their own around it (below), and a block here takes its isize samples from the
// channel's 12 kHz row in12 and leaves isize samples in out12 (both of stride12 doubles per channel), with the same ring indices.
template <bool ROWS>
static __global__ __launch_bounds__(64) void snba_kernel(double2 *buf, long long stride, int nblk, int dsp_size, const int *chan_list,
                                                         SnbaParam q, const double *h_in, const double *h_out, double *state,
                                                         SnbaIdx *idx, double *scratch, const SnbaTune *tune,
                                                         const double *in12, double *out12, long long stride12)
{
#pragma clang fp contract(off)
    __shared__ SnbaLds s;
    __shared__ SnbaRsLds<!ROWS> rs;
    const int ch = chan_list[blockIdx.x], lane = threadIdx.x;
    {
        const SnbaTune t = tune[ch];
        q.asize = t.asize; q.npasses = t.npasses; q.b = t.b; q.pre = t.pre; q.post = t.post; q.k1 = t.k1; q.k2 = t.k2; q.pmultmin = t.pmultmin;
    }
    double2 *row = buf + (long long)ch * stride;
    double *st = state + (size_t)ch * q.state_doubles;
    double *B = scratch + (size_t)ch * kSnbX * kSnbX;
    const double *ho = h_out + (size_t)ch * q.ratio * q.cpp_out;
    const int hin = q.cpp_in - 1, hout = q.cpp_out - 1;
    SnbaIdx ix = idx[ch];
    for (int i = lane; i < 2 * kSnbX; i += 64) s.xb[i] = st[i];
    if (!ROWS) {
        for (int i = lane; i < hin; i += 64) rs.sin_[i] = st[q.off_rin + i];
        for (int i = lane; i < hout; i += 64) rs.sob[i] = st[q.off_rout + i];
    }
    __syncthreads();
    double *inacc = st + q.off_inacc, *outacc = st + q.off_outacc;
    for (int blk = 0; blk < nblk; blk++) {
        double2 *p = row + (long long)blk * dsp_size;
        if (ROWS) {
            const double *p12 = in12 + (long long)ch * stride12 + (long long)blk * q.isize;
            for (int m = lane; m < q.isize; m += 64) inacc[(ix.iainidx + m) % q.iasize] = p12[m];
            __syncthreads();
        } else {
            // xresample (inresamp): L = 1, M = ratio; out[m] = sum_j h[j] x[m * ratio - j]
            for (int i = lane; i < dsp_size; i += 64) rs.sin_[hin + i] = p[i].x;
            __syncthreads();
            for (int m = lane; m < q.isize; m += 64) {
                double acc;
                if (q.ratio == 1) acc = rs.sin_[hin + m];
                else {
                    acc = 0.0;
                    const double *xp = rs.sin_ + hin + m * q.ratio;
                    for (int j = 0; j < q.cpp_in; j++) acc += h_in[j] * xp[-j];
                }
                inacc[(ix.iainidx + m) % q.iasize] = acc;
            }
            __syncthreads();
            for (int base = 0; base < hin; base += 64) {         // slide the input history down by one block
                const double keep = base + lane < hin ? rs.sin_[dsp_size + base + lane] : 0.0;
                __syncthreads();
                if (base + lane < hin) rs.sin_[base + lane] = keep;
                __syncthreads();
            }
        }
        ix.iainidx = (ix.iainidx + q.isize) % q.iasize;
        ix.nsamps += q.isize;
        __syncthreads();
        while (ix.nsamps >= q.incr) {
            for (int i = lane; i < q.incr; i += 64) s.xb[2 * kSnbX - q.incr + i] = inacc[ix.iaoutidx + i];
            __syncthreads();
            snba_frame(s, q, B, lane);
            ix.iaoutidx = (ix.iaoutidx + q.incr) % q.iasize;
            ix.nsamps -= q.incr;
            for (int i = lane; i < q.incr; i += 64) outacc[ix.oainidx + i] = s.xb[kSnbX + i];
            ix.oainidx = (ix.oainidx + q.incr) % q.oasize;
            __syncthreads();
            for (int base = 0; base < 2 * kSnbX - q.incr; base += 64) {      // memmove(xbase, xbase + incr, ...), snb.c:556
                const double keep = base + lane < 2 * kSnbX - q.incr ? s.xb[q.incr + base + lane] : 0.0;
                __syncthreads();
                if (base + lane < 2 * kSnbX - q.incr) s.xb[base + lane] = keep;
                __syncthreads();
            }
        }
        if (ROWS) {
            double *p12 = out12 + (long long)ch * stride12 + (long long)blk * q.isize;
            for (int i = lane; i < q.isize; i += 64) p12[i] = outacc[(ix.oaoutidx + i) % q.oasize];
            ix.oaoutidx = (ix.oaoutidx + q.isize) % q.oasize;
            __syncthreads();
            continue;
        }
        for (int i = lane; i < q.isize; i += 64) rs.sob[hout + i] = outacc[(ix.oaoutidx + i) % q.oasize];
        ix.oaoutidx = (ix.oaoutidx + q.isize) % q.oasize;
        __syncthreads();
        // xresample (outresamp): L = ratio, M = 1; out[i * ratio + ph] = sum_j h[ph][j] o[i - j]
        for (int n = lane; n < dsp_size; n += 64) {
            double acc;
            if (q.ratio == 1) acc = rs.sob[hout + n];
            else {
                const int i = n / q.ratio, ph = n - i * q.ratio;
                const double *hp = ho + ph * q.cpp_out, *op = rs.sob + hout + i;
                acc = 0.0;
                for (int j = 0; j < q.cpp_out; j++) acc += hp[j] * op[-j];
            }
            p[n] = make_double2(acc, 0.0);
        }
        __syncthreads();
        for (int base = 0; base < hout; base += 64) {
            const double keep = base + lane < hout ? rs.sob[q.isize + base + lane] : 0.0;
            __syncthreads();
            if (base + lane < hout) rs.sob[base + lane] = keep;
            __syncthreads();
        }
    }
    for (int i = lane; i < 2 * kSnbX; i += 64) st[i] = s.xb[i];
    if (!ROWS) {
        for (int i = lane; i < hin; i += 64) st[q.off_rin + i] = rs.sin_[i];
        for (int i = lane; i < hout; i += 64) st[q.off_rout + i] = rs.sob[i];
    }
    if (lane == 0) idx[ch] = ix;
}

// ---- the three-pass form's resamplers: xresample (wdsp/resample.c:120-157) as plain FIRs over the whole call ------------------
// A sample g of a pass's input, counted from the first one of this call: the call's own samples from g = 0 on, and the pass's saved
// history (the last `hist` samples of the calls before, oldest first) in front of them.

// outputs per block of the decimation pass: T * ratio = 2048 samples of window beside the cpp_in - 1 of history, at least one
// wavefront and at most four (ratio 32: 64 outputs, 6733 doubles = 53 KB of LDS with the padding below; ratio 16: 128, 36 KB; ratio 8: 256, 28 KB)
static inline int snba_decim_T(int ratio) { const int t = 2048 / ratio; return t < 64 ? 64 : t > 256 ? 256 : t; }

// inresamp: L = 1, M = ratio.  y12[m] = sum_{j = 0 .. cpp_in - 1} h_in[j] x_re[m * ratio - j] for the n12 = nblk * isize outputs of the
// call; block (x, y) takes outputs x * T .. x * T + T - 1 (T = blockDim.x) of listed channel y, their window of T * ratio + cpp_in - 1
// real parts in LDS.  The taps are one array for all channels, read at a wave-uniform index.  The history is only read here.
// The lanes of a wave read samples `ratio` doubles apart, which at ratio 32 is one LDS bank for all of them: window sample w is kept at
// w + w / ratio, one double of padding per `ratio` samples (ratio is a power of two), so that the lanes are ratio + 1 doubles apart.
static inline int snba_decim_lds_doubles(int ratio, int T) { return T * ratio + 140 * ratio + T + 141; }
static __global__ __launch_bounds__(256) void snba_decim_kernel(const double2 *buf, long long stride, int n12, const int *chan_list, SnbaParam q,
                                                                const double *h_in, const double *state, double *out12, long long stride12)
{
#pragma clang fp contract(off)
    extern __shared__ double snba_win[];
    const int ch = chan_list[blockIdx.y], T = blockDim.x, hin = q.cpp_in - 1;
    const int m0 = blockIdx.x * T;
    const int nout = n12 - m0 < T ? n12 - m0 : T;           // outputs of this block (the grid covers n12: at least 1)
    const double2 *row = buf + (long long)ch * stride;
    const double *hist = state + (size_t)ch * q.state_doubles + q.off_rin;
    // window sample w is input g = m0 * ratio - hin + w; the last one needed is that of output m0 + nout - 1
    const long long g0 = (long long)m0 * q.ratio - hin;
    const int nwin = (nout - 1) * q.ratio + 1 + hin, lg = __ffs(q.ratio) - 1;
    for (int w = threadIdx.x; w < nwin; w += T) {
        const long long g = g0 + w;
        snba_win[w + (w >> lg)] = g < 0 ? hist[hin + g] : row[g].x;
    }
    __syncthreads();
    const int m = threadIdx.x;
    if (m >= nout) return;
    double acc;
    if (q.ratio == 1) acc = snba_win[2 * m];
    else {
        // x[m * ratio - j] is window sample hin + m * ratio - j with hin = 140 * ratio: j = 0 is the first sample of padding group 140 + m,
        // j = c * ratio + 1 ... (c + 1) * ratio are group 139 + m - c from its last sample down
        const int top = (140 + m) << lg;
        acc = 0.0;
        acc += h_in[0] * snba_win[top + 140 + m];
        const double *h = h_in + 1;
        for (int c = 0; c < 140; c++) {
            const double *xp = snba_win + (top - (c << lg) - 1) + (139 + m - c);
            for (int i = 0; i < q.ratio; i++) acc += h[i] * xp[-i];
            h += q.ratio;
        }
    }
    out12[(long long)ch * stride12 + m0 + m] = acc;
}

// outresamp: L = ratio, M = 1.  out[i * ratio + ph] = sum_{j = 0 .. 140} h_out[ch][ph][j] o12[i - j] for the n = n12 * ratio samples of the
// call, written as (acc, 0) into the channel's row; block (x, y) takes samples x * 256 .. of listed channel y, its window of
// 256 / ratio (at least 1 ... 256) + 140 samples of the 12 kHz row in LDS.  The taps are the channel's own (SetRXASNBAOutputBandwidth).
static __global__ __launch_bounds__(256) void snba_interp_kernel(double2 *buf, long long stride, int n12, const int *chan_list, SnbaParam q,
                                                                 const double *h_out, const double *state, const double *in12, long long stride12)
{
#pragma clang fp contract(off)
    __shared__ double win[256 + 140];
    const int ch = chan_list[blockIdx.y], hout = q.cpp_out - 1;
    const long long n = (long long)n12 * q.ratio, n0 = (long long)blockIdx.x * 256;
    const int nout = n - n0 < 256 ? (int)(n - n0) : 256;
    const int i0 = (int)(n0 / q.ratio);                      // 256 is a multiple of every ratio: the block starts at phase 0
    const int nwin = (nout - 1) / q.ratio + 1 + hout;
    const double *hist = state + (size_t)ch * q.state_doubles + q.off_rout;
    const double *o12 = in12 + (long long)ch * stride12;
    for (int w = threadIdx.x; w < nwin; w += 256) {
        const int g = i0 - hout + w;
        win[w] = g < 0 ? hist[hout + g] : o12[g];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= nout) return;
    double acc;
    if (q.ratio == 1) acc = win[t];
    else {
        const int i = t / q.ratio, ph = t - i * q.ratio;
        const double *hp = h_out + (size_t)ch * q.ratio * q.cpp_out + ph * q.cpp_out, *op = win + hout + i;
        acc = 0.0;
        for (int j = 0; j < q.cpp_out; j++) acc += hp[j] * op[-j];
    }
    buf[(long long)ch * stride + n0 + t] = make_double2(acc, 0.0);
}

// A pass's history behind it: the last `hist` samples of (old history | the n samples of this call), oldest first, at state offset
// `off` of every listed channel.  src: the call's samples, `step` doubles apart (2: the real parts of a row of the chain buffer,
// 1: a 12 kHz row).  One block per channel; the new history is complete in LDS before any of it is written, as n may be below hist.
static __global__ __launch_bounds__(256) void snba_hist_kernel(const double *src, long long src_stride, int step, int n, const int *chan_list,
                                                               double *state, int state_doubles, int off, int hist)
{
    extern __shared__ double snba_keep[];
    const int ch = chan_list[blockIdx.x];
    double *h = state + (size_t)ch * state_doubles + off;
    const double *x = src + (long long)ch * src_stride;
    for (int i = threadIdx.x; i < hist; i += 256) {
        const long long g = (long long)i + n - hist;         // the sample that becomes history entry i
        snba_keep[i] = g < 0 ? h[hist + g] : x[g * step];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < hist; i += 256) h[i] = snba_keep[i];
}

}  // namespace qh
