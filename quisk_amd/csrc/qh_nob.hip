// qh_nob.hip -- WDSP's second noise blanker NOB (include/quiskhip.h group 10c): xnob and its setters, wdsp/nobII.c:36-155,157-495,
// 650-734, for `nch` fp64 complex streams at the receiver's input rate, every channel with its own settings and state.
//
// The reference keeps one ring of dline_size slots (samples and impulse flags).  Per sample it writes the newest one D slots ahead of
// the one that leaves, flags it (mag > avg threshold, avg stepped first), and a ten-state machine looks at the flag S0 = adv_slew + adv
// + 1 slots ahead of the output: a flag there sets up one blank -- the flags ahead are walked, each impulse stretched by hang +
// hang_slew, sequences closer than adv_slew + adv merged (nobII.c:212-242), two 10-tap sums taken over the clean samples before and
// after -- which the states 1-4 then play out (slew, fill, slew); a sequence longer than max_imp_seq goes through states 5-9 (zeros
// until a whole window of flags is clear).  Positions here are stream indices relative to the call's first sample: at step s the
// newest sample is s, the output is sample s - D, the scan point is s - (D - S0).  The call is cut as qh_anb.hip cuts xanb:
//   det 0 / carry / det 1    the detector of qh_blank_det.hpp: the impulse flags, 64 samples a word           (two reads of the rows)
//   copy     one thread per output sample: the sample D back, from the call's rows or the history             (one read, one write)
//   walk     one wavefront per channel, from event to event: quiet stretches are skipped by bit scans (a __ballot over 64 words), a
//            set-up does the reference's merging loop with a dilation of the flags by hang + hang_slew + 1 and bit scans, gathers the
//            FIR taps by bit scans, and the 64 lanes write the slews, the fill or the zeros of the blank over the copy.  A mode-4 fill
//            is the reference's repeated addition, stepped serially (every lane steps it, lane k & 63 stores): its cost grows with
//            the blanked samples of that mode only
//   hist     the last kNobHist samples and flags of every running channel to the other history buffers
// A read of the reference that runs ahead of its write position (the look-ahead, the forward gather) finds the slot as it was
// dline_size samples earlier: position u > s means u - dline_size (nob_bits64, nob_samp), which is why a channel keeps dline_size
// samples and flags of history.  bfbuff is rebuilt at each set-up from the flags and samples behind it.
// Given the flags (see the header for where they can differ from a sample-serial run) the output is the reference's bit for bit: the
// tables, backmult and the counts come from the host's C library, the sums and products are the reference's in its order.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>
#include "qh_blank_det.hpp"

#pragma clang fp contract(off)

using namespace qh;

namespace {

constexpr double kNobMaxTime = 0.002, kNobMaxSeqTime = 0.025, kNobMaxRate = 1536000.0;     // nobII.c:29-34
constexpr int kNobSize = (int)(kNobMaxRate * (kNobMaxTime + kNobMaxTime + kNobMaxTime + kNobMaxTime + kNobMaxSeqTime) + 2);    // dline_size, nobII.c:94-98
constexpr int kNobHW = (kNobSize + 63) / 64;            // words of flags kept per channel
constexpr int kNobHist = kNobHW * 64;                   // samples kept per channel
constexpr int kNobWave = (int)(kNobMaxTime * kNobMaxRate + 1);     // doubles of awave[] / hwave[] per channel, nobII.c:101-102
constexpr int kNobTaps = 10;                            // filterlen, nobII.c:104
constexpr long long kNobAll = LLONG_MAX / 4;            // "everything asked for has been written"
constexpr long long kNobNone = LLONG_MAX;

struct NobParam {
    double backmult, ombackmult, threshold;
    double carry;                       // backmult^kDetL
    int asl, adv, hang, hsl, mseq;      // adv_slew_count, adv_count, hang_count, hang_slew_count, max_imp_seq
    int D, mode, run;
};
static_assert(sizeof(NobParam) == 64, "the layout the kernels and the upload share");

// what xnob keeps from call to call, but for the ring (the history buffers) and bfbuff (rebuilt)
struct NobState {
    double avg, I, Q, dI, dQ, Il, Ql, In, Qn;
    int S, tm, blank, pad;
};
static_assert(sizeof(NobState) == 88, "the layout the kernels share");

// One channel's samples and flags as the walk sees them: positions >= 0 are the call's (flags in tw, nw words), positions in
// [-kNobHist, 0) the history's; older ones read as the flush's zeros.
struct NobCtx {
    const double2 *in, *hist;
    const u64 *tw, *hb;
    long long n, nw;
};

__device__ __forceinline__ u64 nob_word(const NobCtx &c, long long W)       // the flags of positions [64 W, 64 W + 64)
{
    if (W >= c.nw) return 0ull;
    if (W >= 0) return c.tw[W];
    return W >= -kNobHW ? c.hb[kNobHW + W] : 0ull;
}

__device__ __forceinline__ u64 nob_raw64(const NobCtx &c, long long q)      // the flags of positions [q, q + 64)
{
    const long long W = q >> 6;
    const int sh = (int)(q & 63);
    u64 r = nob_word(c, W) >> sh;
    if (sh) r |= nob_word(c, W + 1) << (64 - sh);
    return r;
}

// the flags the reference finds at positions [u0, u0 + 64) when its newest sample is s: a position beyond s is a slot not yet
// rewritten, dline_size samples old
__device__ u64 nob_bits64(const NobCtx &c, long long u0, long long s)
{
    if (u0 + 63 <= s) return nob_raw64(c, u0);
    u64 r = 0ull;
    for (int got = 0; got < 64;) {
        long long u = u0 + got;
        while (u > s) u -= kNobSize;
        const long long room = s - u + 1;
        const int take = room < 64 - got ? (int)room : 64 - got;
        u64 w = nob_raw64(c, u);
        if (take < 64) w &= (1ull << take) - 1ull;
        r |= w << got;
        got += take;
    }
    return r;
}

__device__ double2 nob_samp(const NobCtx &c, long long u, long long s)
{
    while (u > s) u -= kNobSize;
    if (u >= 0) return c.in[u];
    return u >= -kNobHist ? c.hist[kNobHist + u] : make_double2(0.0, 0.0);
}

// the first position in [lo, hi] whose flag is set (clear, with `clear`), kNobNone if none; the whole wavefront, 64 words a trip
__device__ long long nob_first(const NobCtx &c, long long lo, long long hi, long long s, bool clear, int lane)
{
    for (long long base = lo & ~63ll; base <= hi; base += 4096) {
        const long long u0 = base + 64 * lane;
        u64 w = 0ull;
        if (u0 <= hi && u0 + 63 >= lo) {
            w = nob_bits64(c, u0, s);
            if (clear) w = ~w;
            if (u0 < lo) w &= ~0ull << (lo - u0);
            if (hi - u0 < 63) w &= (1ull << (hi - u0 + 1)) - 1ull;
        }
        const u64 bal = __ballot(w != 0ull);
        if (bal) {
            const int l0 = __ffsll((long long)bal) - 1;
            const u64 wl = __shfl(w, l0, 64);
            return base + 64 * l0 + __ffsll((long long)wl) - 1;
        }
    }
    return kNobNone;
}

// the last position in [lo, hi] whose flag is set, kNobNone if none
__device__ long long nob_last(const NobCtx &c, long long lo, long long hi, long long s, int lane)
{
    for (long long top = hi; top >= lo; top -= 4096) {
        const long long u0 = top - 63 - 64 * lane;
        u64 w = 0ull;
        if (u0 + 63 >= lo) {
            w = nob_bits64(c, u0, s);
            if (u0 < lo) w &= ~0ull << (lo - u0);
        }
        const u64 bal = __ballot(w != 0ull);
        if (bal) {
            const int l0 = __ffsll((long long)bal) - 1;
            const u64 wl = __shfl(w, l0, 64);
            return top - 64 * l0 - __clzll((long long)wl);
        }
    }
    return kNobNone;
}

// The inner while of nobII.c:216-222 from a set flag at p: the first position e > p with no flag in [e - G, e] (every impulse holds
// the loop for G = hang + hang_slew more samples), but no further than p + cap.
__device__ long long nob_run_end(const NobCtx &c, long long p, long long cap, int G, long long s, int lane)
{
    long long lt = LLONG_MIN / 2;                       // the last flag so far
    for (long long base = p; base - p < cap; base += 4096) {
        const long long ws = base + 64 * lane;
        const u64 tw = ws - p < cap ? nob_bits64(c, ws, s) : 0ull;
        long long inc = tw ? ws + 63 - __clzll((long long)tw) : LLONG_MIN / 2;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(inc, d, 64);
            if (lane >= d && up > inc) inc = up;
        }
        const long long ex = __shfl_up(inc, 1, 64);
        const long long ltb = lane && ex > lt ? ex : lt;
        u64 cov = dilate(tw, G + 1);
        const long long left = (long long)G + 1 - (ws - ltb);               // bits of the word a flag before it still holds
        if (left > 0) cov |= left >= 64 ? ~0ull : (1ull << left) - 1ull;
        const u64 bal = __ballot(~cov != 0ull);
        if (bal) {
            const int l0 = __ffsll((long long)bal) - 1;
            const u64 z = __shfl(~cov, l0, 64);
            const long long e = base + 64 * l0 + __ffsll((long long)z) - 1;
            return e - p < cap ? e : p + cap;
        }
        const long long top = __shfl(inc, 63, 64);
        if (top > lt) lt = top;
    }
    return p + cap;
}

// The ten clean samples at and before (dir < 0) or at and after (dir > 0) position u, nearest first, through the reference's sum
// (nobII.c:254-259, 280-285): fcoefs[0] on the nearest.
__device__ double2 nob_fir(const NobCtx &c, long long u, int dir, long long s, int lane)
{
    const double f[kNobTaps] = { 0.308720593, 0.216104415, 0.151273090, 0.105891163, 0.074123814,
                                 0.051886670, 0.036320669, 0.025424468, 0.017797128, 0.012457989 };     // nobII.c:108-117
    int cnt = 0;
    long long mine = 0;
    // Positions older than the history read as clean zeros, so the backward gather ends.  The forward one sees the ring's flags
    // again after kNobSize positions: it stops there, and the taps it has not found are zeros (the reference's loop would not end).
    for (long long edge = u; cnt < kNobTaps && (dir < 0 || edge - u < kNobSize); edge += dir * 4096) {
        const long long u0 = dir < 0 ? edge - 63 - 64 * lane : edge + 64 * lane;
        u64 w = 0ull;
        const long long room = dir < 0 ? 64 : kNobSize - (u0 - u);         // positions of this word inside one turn of the ring
        if (room > 0) {
            w = ~nob_bits64(c, u0, s);
            if (room < 64) w &= (1ull << room) - 1ull;
        }
        for (u64 bal = __ballot(w != 0ull); bal && cnt < kNobTaps; bal &= bal - 1ull) {     // lane order is nearest first
            const int l = __ffsll((long long)bal) - 1;
            u64 wl = __shfl(w, l, 64);
            const long long b0 = dir < 0 ? edge - 63 - 64 * l : edge + 64 * l;
            while (wl && cnt < kNobTaps) {
                const int b = dir < 0 ? 63 - __clzll((long long)wl) : __ffsll((long long)wl) - 1;
                if (lane == cnt) mine = b0 + b;
                cnt++;
                wl &= ~(1ull << b);
            }
        }
    }
    const double2 v = lane < cnt ? nob_samp(c, mine, s) : make_double2(0.0, 0.0);
    double I = 0.0, Q = 0.0;
    for (int k = 0; k < kNobTaps; k++) {
        const double a = __shfl(v.x, k, 64), b = __shfl(v.y, k, 64);
        I += f[k] * a;
        Q += f[k] * b;
    }
    return make_double2(I, Q);
}

// One thread per output sample: the sample D back (nobII.c:197-198); a channel with run = 0 copies (nobII.c:492-493).
__global__ __launch_bounds__(256) void nob_copy_kernel(const double2 *in, long long in_stride, double2 *out, long long out_stride, int n,
                                                       const NobParam *prm, const double2 *hist)
{
    const int ch = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 *irow = in + (long long)ch * in_stride;
    const long long D = prm[ch].run ? prm[ch].D : 0;
    out[(long long)ch * out_stride + i] = i >= D ? irow[i - D] : hist[(long long)ch * kNobHist + (kNobHist + (i - D))];
}

// The event walk, one wavefront per channel.  Every lane holds the machine (the control flow is uniform); the lanes share the bit
// scans and the stores.
__global__ __launch_bounds__(64) void nob_walk_kernel(const double2 *in, long long in_stride, double2 *out, long long out_stride, int n,
                                                      const NobParam *prm, NobState *state, const double *awave, const double *hwave,
                                                      const double2 *hist, const u64 *trb, long long wstride, const u64 *hbits)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    const NobParam p = prm[ch];
    if (!p.run) return;
    NobState st = state[ch];
    NobCtx c;
    c.in = in + (long long)ch * in_stride;
    c.hist = hist + (long long)ch * kNobHist;
    c.tw = trb + (long long)ch * wstride;
    c.hb = hbits + (long long)ch * kNobHW;
    c.n = n;
    c.nw = ((long long)n + 63) / 64;
    double2 *o = out + (long long)ch * out_stride;
    const double *aw = awave + (long long)ch * kNobWave, *hw = hwave + (long long)ch * kNobWave;
    const int asl = p.asl, adv = p.adv, hang = p.hang, hsl = p.hsl, mseq = p.mseq;
    const long long D = p.D, Lk = D - (asl + adv + 1), N = n;
    // states 8 and 7 leave for 9 with the sample that follows the rise (nobII.c:437-440, 460-463), or for 0
    auto leave_overflow = [&](long long s) {
        if (hsl > 0) {
            const double2 v = nob_samp(c, s + 1 + hsl - D, s);
            st.In = v.x; st.Qn = v.y; st.S = 9;
        } else st.S = 0;
    };
    long long pp = 0;
    while (pp < N) {
        const int S = st.S;
        if (S == 0) {
            const long long q = nob_first(c, pp - Lk, N - 1 - Lk, kNobAll, false, lane);
            if (q == kNobNone) break;
            const long long s = q + Lk;                                     // the set-up, nobII.c:201-333
            pp = s + 1;
            const double2 last = nob_samp(c, s - D, s);
            st.Il = last.x; st.Ql = last.y;
            st.tm = 0;
            st.S = asl > 0 ? 1 : adv > 0 ? 2 : 3;
            long long t = q;
            int blank = 0;
            bool over = false;
            for (;;) {
                const int cap = mseq - blank;
                if (cap > 0) {
                    const long long e = nob_run_end(c, t, cap, hang + hsl, s, lane);
                    blank += (int)(e - t);
                    t = e;
                }
                int len = 0;
                if (asl + adv > 0) {
                    const long long f = nob_first(c, t, t + asl + adv - 1, s, false, lane);
                    if (f != kNobNone) { len = (int)(f - t) + 1; t = f; }
                }
                blank += len;
                if (blank > mseq) { blank = mseq; over = true; break; }
                if (len == 0) break;
            }
            if (over) {
                st.blank = blank;
                if (asl > 0) st.S = 5;
                else { st.S = 6; st.blank += adv + kNobTaps; }
                continue;
            }
            blank -= hsl;
            st.blank = blank;
            const double2 nx = nob_samp(c, t, s);
            st.In = nx.x; st.Qn = nx.y;
            double2 f1 = make_double2(0.0, 0.0), f2 = f1;
            if (p.mode == 1 || p.mode == 2 || p.mode == 4) f1 = nob_fir(c, s - D + asl, -1, s, lane);
            if (p.mode == 2 || p.mode == 3 || p.mode == 4) f2 = nob_fir(c, q + blank, 1, s, lane);
            st.dI = 0.0; st.dQ = 0.0;
            if (p.mode == 0) { st.I = 0.0; st.Q = 0.0; }
            else if (p.mode == 1) { st.I = f1.x; st.Q = f1.y; }
            else if (p.mode == 2) { st.I = 0.5 * (f1.x + f2.x); st.Q = 0.5 * (f1.y + f2.y); }
            else if (p.mode == 3) { st.I = f2.x; st.Q = f2.y; }
            else {
                st.dI = (f2.x - f1.x) / (adv + blank);
                st.dQ = (f2.y - f1.y) / (adv + blank);
                st.I = f1.x; st.Q = f1.y;
            }
        } else if (S == 1 || S == 5) {                                      // nobII.c:336-350, 393-405
            const long long end = pp + (asl - st.tm) < N ? pp + (asl - st.tm) : N;
            for (long long k = pp + lane; k < end; k += 64) {
                const double scale = 0.5 + aw[st.tm + (k - pp)];
                o[k] = S == 1 ? make_double2(st.Il * scale + (1.0 - scale) * st.I, st.Ql * scale + (1.0 - scale) * st.Q)
                              : make_double2(st.Il * scale, st.Ql * scale);
            }
            st.tm += (int)(end - pp);
            pp = end;
            if (st.tm == asl) {
                st.tm = 0;
                if (S == 1) st.S = adv > 0 ? 2 : 3;
                else { st.S = 6; st.blank += adv + kNobTaps; }
            }
        } else if (S == 2 || S == 3) {                                      // nobII.c:351-383
            const int len = S == 2 ? adv : st.blank;
            const long long end = pp + (len - st.tm) < N ? pp + (len - st.tm) : N;
            if (st.dI == 0.0 && st.dQ == 0.0) {
                for (long long k = pp + lane; k < end; k += 64) o[k] = make_double2(st.I, st.Q);
            } else {
                for (long long k = pp; k < end; k++) {                      // I += deltaI, once per sample
                    if (((k - pp) & 63) == lane) o[k] = make_double2(st.I, st.Q);
                    st.I += st.dI;
                    st.Q += st.dQ;
                }
            }
            st.tm += (int)(end - pp);
            pp = end;
            if (st.tm == len) {
                st.tm = 0;
                st.S = S == 2 ? 3 : hsl > 0 ? 4 : 0;
            }
        } else if (S == 4 || S == 9) {                                      // nobII.c:384-392, 473-485
            const long long end = pp + (hsl - st.tm) < N ? pp + (hsl - st.tm) : N;
            for (long long k = pp + lane; k < end; k += 64) {
                const double scale = 0.5 - hw[st.tm + (k - pp)];
                o[k] = S == 4 ? make_double2(st.In * scale + (1.0 - scale) * st.I, st.Qn * scale + (1.0 - scale) * st.Q)
                              : make_double2(st.In * scale, st.Qn * scale);
            }
            st.tm += (int)(end - pp);
            pp = end;
            if (st.tm >= hsl) { st.tm = 0; st.S = 0; }
        } else if (S == 6 || S == 8) {                                      // nobII.c:406-413, 450-472
            const int len = S == 6 ? st.blank : hang;
            const long long end = pp + (len - st.tm) < N ? pp + (len - st.tm) : N;
            for (long long k = pp + lane; k < end; k += 64) o[k] = make_double2(0.0, 0.0);
            st.tm += (int)(end - pp);
            pp = end;
            if (st.tm == len) {
                st.tm = 0;
                if (S == 6) st.S = 7;
                else leave_overflow(pp - 1);
            }
        } else {                                                            // 7, nobII.c:414-449: the first step whose window is clear
            long long s = pp;
            while (s < N) {
                const long long l = nob_last(c, s - D + 1, s - Lk + hsl + hang, kNobAll, lane);      // adv + adv_slew + hang_slew + hang + 1 flags
                if (l == kNobNone) break;
                s = l + D;
            }
            const long long end = s < N ? s + 1 : N;
            for (long long k = pp + lane; k < end; k += 64) o[k] = make_double2(0.0, 0.0);
            pp = end;
            if (s < N) {
                st.tm = 0;
                if (hang > 0) st.S = 8;
                else leave_overflow(s);
            }
        }
    }
    if (lane == 0) {
        st.avg = state[ch].avg;                                             // det 1's
        state[ch] = st;
    }
}

// new history <- the last kNobHist samples and flags of the stream of a running channel; a channel that does not run keeps its own
__global__ __launch_bounds__(256) void nob_hist_kernel(const double2 *in, long long in_stride, int n, const NobParam *prm, const double2 *old_hist,
                                                       double2 *new_hist, const u64 *trb, long long wstride, const u64 *old_bits, u64 *new_bits)
{
    const int ch = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= kNobHist) return;
    const long long g = (long long)n - kNobHist + j, row = (long long)ch * kNobHist;
    const bool run = prm[ch].run != 0;
    double2 v;
    if (!run) v = old_hist[row + j];
    else v = g >= 0 ? in[(long long)ch * in_stride + g] : old_hist[row + (kNobHist + g)];
    new_hist[row + j] = v;
    if (j < kNobHW) {
        NobCtx c;
        c.in = nullptr; c.hist = nullptr;
        c.tw = trb + (long long)ch * wstride;
        c.hb = old_bits + (long long)ch * kNobHW;
        c.n = n;
        c.nw = ((long long)n + 63) / 64;
        new_bits[(long long)ch * kNobHW + j] = run ? nob_raw64(c, (long long)n - kNobHist + 64ll * j) : c.hb[j];
    }
}

// flush_nob (nobII.c:141-155) for channels ch0 .. ch0 + gridDim.y - 1: the detector and the machine start over, the ring is zeroed
__global__ __launch_bounds__(256) void nob_reset_kernel(NobState *state, double2 *hist, u64 *bits, int ch0)
{
    const int ch = ch0 + blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j < kNobHist) hist[(long long)ch * kNobHist + j] = make_double2(0.0, 0.0);
    if (j < kNobHW) bits[(long long)ch * kNobHW + j] = 0ull;
    if (j == 0) { NobState &s = state[ch]; s.avg = 1.0; s.S = 0; }
}

struct NobSettings {
    double samplerate, slewtime, hangtime, advtime, backtau, threshold;
    int mode, run;
};

struct NobCounts { int asl, adv, hang, hsl, mseq, D; };

NobCounts nob_counts(const NobSettings &s)              // init_nob, nobII.c:40-44; flush_nob, nobII.c:143-145
{
    NobCounts c;
    c.asl = (int)(s.slewtime * s.samplerate);
    c.adv = (int)(s.advtime * s.samplerate);
    c.hang = (int)(s.hangtime * s.samplerate);
    c.hsl = (int)(s.slewtime * s.samplerate);
    c.mseq = (int)(kNobMaxSeqTime * s.samplerate);
    c.D = c.asl + c.adv + 1 + c.mseq + c.hang + c.hsl + kNobTaps;
    return c;
}

const char *nob_refusal(const NobSettings &s)
{
    if (!(s.samplerate > 0.0 && s.samplerate <= kNobMaxRate)) return "the sample rate must lie in (0, 1536000]";
    if (!(s.slewtime >= 0.0 && s.slewtime <= kNobMaxTime)) return "the slew time must lie in [0, 0.002]";
    if (!(s.hangtime >= 0.0 && s.hangtime <= kNobMaxTime)) return "hangtime must lie in [0, 0.002]";
    if (!(s.advtime >= 0.0 && s.advtime <= kNobMaxTime)) return "advtime must lie in [0, 0.002]";
    if (!(s.backtau > 0.0) || !std::isfinite(s.backtau)) return "backtau must be finite and positive";
    if (!std::isfinite(s.threshold)) return "the threshold must be finite";
    if (s.mode < 0 || s.mode > 4) return "the mode must lie in 0 .. 4";
    const NobCounts c = nob_counts(s);
    if (c.mseq < 1) return "the sample rate must give max_imp_seq_time (0.025 s) at least one sample";
    if (c.D >= kNobSize) return "the delay would reach the ring's length (the reference then writes beyond its delay line)";
    return nullptr;
}

}  // namespace

int qh::nob_check_settings(double samplerate, int mode, double slewtime, double hangtime, double advtime, double backtau, double threshold)
{
    const char *why = nob_refusal(NobSettings{samplerate, slewtime, hangtime, advtime, backtau, threshold, mode, 1});
    return why ? set_error(QH_ERR_INVALID, "%s", why) : QH_OK;
}

struct qh_nob : DetBank {
    std::vector<NobSettings> set;
    std::vector<NobParam> prm;
    std::vector<double> awave, hwave;                   // [nch][kNobWave]
    std::vector<char> wave_dirty;
    NobParam *d_prm = nullptr;
    NobState *d_state = nullptr;
    double *d_awave = nullptr, *d_hwave = nullptr;
    double2 *hist[2] = { nullptr, nullptr };
    u64 *bits[2] = { nullptr, nullptr };
    ~qh_nob()
    {
        quiesce();
        (void)hipFree(d_prm); (void)hipFree(d_state); (void)hipFree(d_awave); (void)hipFree(d_hwave);
        (void)hipFree(hist[0]); (void)hipFree(hist[1]); (void)hipFree(bits[0]); (void)hipFree(bits[1]);
    }

    static const char *refusal(const NobSettings &s) { return nob_refusal(s); }

    // init_nob's numbers (nobII.c:40-58), with the C library's exp and cos
    void derive(int ch)
    {
        const NobSettings &s = set[ch];
        NobParam &p = prm[ch];
        const NobCounts c = nob_counts(s);
        p.asl = c.asl; p.adv = c.adv; p.hang = c.hang; p.hsl = c.hsl; p.mseq = c.mseq; p.D = c.D;
        p.backmult = std::exp(-1.0 / (s.samplerate * s.backtau));
        p.ombackmult = 1.0 - p.backmult;
        p.carry = std::pow(p.backmult, (double)kDetL);
        p.threshold = s.threshold;
        p.mode = s.mode;
        p.run = s.run;
        const double PI = 3.1415926535897932;               // comm.h
        double *a = awave.data() + (size_t)ch * kNobWave, *w = hwave.data() + (size_t)ch * kNobWave;
        if (p.asl > 0) {
            const double coef = PI / (p.asl + 1);
            for (int i = 0; i < p.asl; i++) a[i] = 0.5 * std::cos((i + 1) * coef);
        }
        if (p.hsl > 0) {
            const double coef = PI / p.hsl;
            for (int i = 0; i < p.hsl; i++) w[i] = 0.5 * std::cos(i * coef);
        }
        wave_dirty[ch] = 1;
        dirty = true;
    }

    void apply_light(int ch) { prm[ch].threshold = set[ch].threshold; prm[ch].run = set[ch].run; prm[ch].mode = set[ch].mode; }

    int restart(int ch0, int count)
    {
        hipLaunchKernelGGL(nob_reset_kernel, dim3((kNobHist + 255) / 256, (unsigned)count), dim3(256), 0, stream, d_state, hist[cur], bits[cur], ch0);
        QH_HIP(hipGetLastError());
        return QH_OK;
    }

    // host settings -> device, behind everything enqueued so far (the copies are synchronous: the vectors may change right after)
    int upload()
    {
        if (!dirty) return QH_OK;
        QH_HIP(hipStreamSynchronize(stream));
        QH_HIP(hipMemcpy(d_prm, prm.data(), (size_t)nch * sizeof(NobParam), hipMemcpyHostToDevice));
        for (int ch = 0; ch < nch; ch++) {
            if (!wave_dirty[ch]) continue;
            if (prm[ch].asl > 0)
                QH_HIP(hipMemcpy(d_awave + (size_t)ch * kNobWave, awave.data() + (size_t)ch * kNobWave, (size_t)prm[ch].asl * sizeof(double),
                                 hipMemcpyHostToDevice));
            if (prm[ch].hsl > 0)
                QH_HIP(hipMemcpy(d_hwave + (size_t)ch * kNobWave, hwave.data() + (size_t)ch * kNobWave, (size_t)prm[ch].hsl * sizeof(double),
                                 hipMemcpyHostToDevice));
            wave_dirty[ch] = 0;
        }
        dirty = false;
        return QH_OK;
    }
};

extern "C" {

qh_nob *qh_nob_create(int device, int nch, double samplerate, int mode, double slewtime, double hangtime, double advtime, double backtau,
                      double threshold, void *stream)
{
    const NobSettings s0{samplerate, slewtime, hangtime, advtime, backtau, threshold, mode, 1};
    if (nch <= 0) { set_error(QH_ERR_INVALID, "qh_nob_create: bad arguments"); return nullptr; }
    if (const char *why = nob_refusal(s0)) { set_error(QH_ERR_INVALID, "qh_nob_create: %s", why); return nullptr; }
    qh_nob *h = new qh_nob();
    h->nch = nch;
    auto fail = [&](const char *what) -> qh_nob * { set_error(QH_ERR_HIP, "qh_nob_create: %s failed", what); delete h; return nullptr; };
    if (bank_open(h, device, stream, "qh_nob_create") != QH_OK) { delete h; return nullptr; }
    h->set.assign((size_t)nch, s0);
    h->prm.assign((size_t)nch, NobParam{});
    h->awave.assign((size_t)nch * kNobWave, 0.0);
    h->hwave.assign((size_t)nch * kNobWave, 0.0);
    h->wave_dirty.assign((size_t)nch, 1);
    h->derive(0);
    for (int ch = 1; ch < nch; ch++) {
        h->prm[ch] = h->prm[0];
        std::copy(h->awave.begin(), h->awave.begin() + kNobWave, h->awave.begin() + (size_t)ch * kNobWave);
        std::copy(h->hwave.begin(), h->hwave.begin() + kNobWave, h->hwave.begin() + (size_t)ch * kNobWave);
    }
    const size_t hb = (size_t)nch * kNobHist, bw = (size_t)nch * kNobHW;
    if (dev_alloc(&h->d_prm, (size_t)nch) != hipSuccess || dev_alloc(&h->d_state, (size_t)nch) != hipSuccess ||
        dev_alloc(&h->d_awave, (size_t)nch * kNobWave) != hipSuccess || dev_alloc(&h->d_hwave, (size_t)nch * kNobWave) != hipSuccess ||
        dev_alloc(&h->hist[0], hb) != hipSuccess || dev_alloc(&h->hist[1], hb) != hipSuccess || dev_alloc(&h->bits[0], bw) != hipSuccess ||
        dev_alloc(&h->bits[1], bw) != hipSuccess)
        return fail("hipMalloc");
    // the allocation of the reference is zeroed (malloc0, nobII.c:80): time, blank_count, I, Q and the deltas start at 0
    if (dev_zero(h->d_state, (size_t)nch * sizeof(NobState)) != hipSuccess || dev_zero(h->d_awave, (size_t)nch * kNobWave * sizeof(double)) != hipSuccess ||
        dev_zero(h->d_hwave, (size_t)nch * kNobWave * sizeof(double)) != hipSuccess || dev_zero(h->hist[1], hb * sizeof(double2)) != hipSuccess ||
        dev_zero(h->bits[1], bw * sizeof(u64)) != hipSuccess)
        return fail("hipMemset");
    if (h->restart(0, nch) != QH_OK) { delete h; return nullptr; }
    return h;
}

void qh_nob_destroy(qh_nob *h) { delete h; }

int qh_nob_delay(qh_nob *h, int ch)
{
    if (!h || ch < 0 || ch >= h->nch) return 0;
    std::lock_guard<std::mutex> lk(h->mtx);
    return h->prm[ch].D;
}

int qh_nob_set_run(qh_nob *h, int ch, int run) { return bank_set(h, ch, "qh_nob_set_run", false, [=](NobSettings &s) { s.run = run != 0; }); }
int qh_nob_set_mode(qh_nob *h, int ch, int mode) { return bank_set(h, ch, "qh_nob_set_mode", false, [=](NobSettings &s) { s.mode = mode; }); }
int qh_nob_set_samplerate(qh_nob *h, int ch, double samplerate) { return bank_set(h, ch, "qh_nob_set_samplerate", true, [=](NobSettings &s) { s.samplerate = samplerate; }); }
int qh_nob_set_tau(qh_nob *h, int ch, double tau) { return bank_set(h, ch, "qh_nob_set_tau", true, [=](NobSettings &s) { s.slewtime = tau; }); }
int qh_nob_set_hangtime(qh_nob *h, int ch, double hangtime) { return bank_set(h, ch, "qh_nob_set_hangtime", true, [=](NobSettings &s) { s.hangtime = hangtime; }); }
int qh_nob_set_advtime(qh_nob *h, int ch, double advtime) { return bank_set(h, ch, "qh_nob_set_advtime", true, [=](NobSettings &s) { s.advtime = advtime; }); }
int qh_nob_set_backtau(qh_nob *h, int ch, double backtau) { return bank_set(h, ch, "qh_nob_set_backtau", true, [=](NobSettings &s) { s.backtau = backtau; }); }
int qh_nob_set_threshold(qh_nob *h, int ch, double threshold) { return bank_set(h, ch, "qh_nob_set_threshold", false, [=](NobSettings &s) { s.threshold = threshold; }); }
int qh_nob_flush(qh_nob *h, int ch) { return bank_set(h, ch, "qh_nob_flush", true, [](NobSettings &) {}); }

int qh_nob_process(qh_nob *h, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n)
{
    if (int rc = bank_check_rows("qh_nob_process", h, d_in, in_stride, d_out, out_stride, n, "an output is the input D samples back")) return rc;
    if (n == 0) return QH_OK;
    std::lock_guard<std::mutex> lk(h->mtx);
    QH_HIP(hipSetDevice(h->device));
    if (int rc = h->upload()) return rc;
    if (int rc = bank_grow(h, n, kDetL, "qh_nob_process")) return rc;
    const double2 *in = static_cast<const double2 *>(d_in);
    double2 *out = static_cast<double2 *>(d_out);
    const long long nw = h->nw;
    const unsigned nch = (unsigned)h->nch;
    bool any = false;
    for (const NobParam &p : h->prm) any = any || p.run;
    hipStream_t s = h->stream;
    if (any) det_enqueue(*h, in, in_stride, n, h->d_prm, h->d_state);
    hipLaunchKernelGGL(nob_copy_kernel, dim3((unsigned)((n + 255) / 256), nch), dim3(256), 0, s, in, in_stride, out, out_stride, n, h->d_prm,
                       h->hist[h->cur]);
    if (any) {
        hipLaunchKernelGGL(nob_walk_kernel, dim3(nch), dim3(64), 0, s, in, in_stride, out, out_stride, n, h->d_prm, h->d_state, h->d_awave, h->d_hwave,
                           h->hist[h->cur], h->d_trb, nw, h->bits[h->cur]);
        hipLaunchKernelGGL(nob_hist_kernel, dim3((kNobHist + 255) / 256, nch), dim3(256), 0, s, in, in_stride, n, h->d_prm, h->hist[h->cur],
                           h->hist[h->cur ^ 1], h->d_trb, nw, h->bits[h->cur], h->bits[h->cur ^ 1]);
        h->cur ^= 1;
    }
    QH_HIP(hipGetLastError());
    return QH_OK;
}

int qh_nob_process_host(qh_nob *h, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n)
{
    return bank_process_host(h, h_in, in_stride, h_out, out_stride, n, qh_nob_process, "qh_nob_process_host");
}

int qh_nob_synchronize(qh_nob *h) { return bank_synchronize(h, "qh_nob_synchronize"); }

}  // extern "C"
