// qh_fmsq.hpp -- xfmsq of xrxa (wdsp/RXA.c:575, wdsp/fmsq.c:141-205): the FM noise squelch, per listed channel, state carried from
// call to call.
//
// The trigger is xfmd's audio ahead of de-emphasis (fmd.c:169-171).  Its noise filter is an ordinary fircore stage of the engine
// (Engine::run_fm: one overlap-save pass with the stage's own mask and delay lines, two channels a tile where the audio is made in the
// load); what this header holds is everything behind it, in one kernel, one wavefront per listed channel, 64 samples per step:
//   noise     sqrt (n0^2 + n1^2) of the filter's output, as written there (fmsq.c:150)
//   averages  avnoise (tau 1 ms) and longnoise (tau 100 ms): two one-pole recurrences, a wave scan (scan_pole_dpp) from zero plus the
//             carried value times m^(lane + 1); the loads and scans of four steps are in flight together
//   bits      avnoise < unmute_thresh and avnoise > tail_thresh of the 64 samples as two words (__ballot); the ready delay as a third
//   machine   the five states (fmsq.c:156-200) walked from event to event over the words with bit scans: a step holds at most a few
//             state changes, and no sample is visited one by one
//   apply     lane i holds the gain of sample i: 0 stored for a MUTED sample, the ramps' table values multiplied in, 1 left alone
// This is AMSQ's one-wavefront-per-channel form (qh_demod.hpp) without its per-sample loop, not SSQL's split over time tiles: a call's
// cost grows with its length per channel and does not spread over the chip (DESIGN.md section 7 and profiles/fmsq_config4.md have the
// measured cost).
// The averages of a step start from the carried values, so they agree with the reference's sample-by-sample recurrence to rounding
// (a few 1e-16 relative), not bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "qh_wave.hpp"

namespace qh {

enum : int { FQ_MUTED, FQ_INCREASE, FQ_UNMUTED, FQ_TAIL, FQ_DECREASE };

struct FmsqParam {
    double avm, onem_avm, longavm, onem_longavm;        // calc_fmsq, fmsq.c:48-52
    double tail_thresh, unmute_thresh, min_tail, max_tail, rate;
    int ntup, ntdown;
};

// wait: the samples still to come until `ready` is set, the one that sets it included (0: ready).  count is not touched by a flush,
// as in flush_fmsq.
struct FmsqState { double avnoise, longnoise; int state, count, wait; };

static constexpr int kFqBatch = 4;      // steps whose loads and scans are in flight together

static __global__ __launch_bounds__(64) void fmsq_kernel(double2 *rows, long long stride, int n, const int *list, const double2 *noise,
                                                         long long nstride, const FmsqParam *prm, FmsqState *state, const double *cup,
                                                         const double *cdown)
{
#pragma clang fp contract(off)
    const int ch = list[blockIdx.x], lane = threadIdx.x;
    const FmsqParam q = prm[ch];
    const FmsqState st = state[ch];
    double2 *p = rows + (long long)ch * stride;
    const double2 *nz = noise + (long long)ch * nstride;
    const PoleScan pa = make_pole_scan(q.avm, lane), pl = make_pole_scan(q.longavm, lane);
    // the machine's variables are the same in every lane: kept in scalar registers, so that the walk below branches on scalars
    int S = __builtin_amdgcn_readfirstlane(st.state), c = __builtin_amdgcn_readfirstlane(st.count), wait = __builtin_amdgcn_readfirstlane(st.wait);
    double avc = st.avnoise, lgc = st.longnoise;            // the averages behind the last sample done
    double2 ahead[kFqBatch];
#pragma unroll
    for (int j = 0; j < kFqBatch; j++) ahead[j] = 64 * j + lane < n ? nz[64 * j + lane] : make_double2(0.0, 0.0);
    for (int base0 = 0; base0 < n; base0 += 64 * kFqBatch) {
        // kFqBatch steps' magnitudes and zero-start scans at once (they do not depend on the carried averages), the batch behind them on
        // its way meanwhile
        double sa[kFqBatch], sl[kFqBatch];
#pragma unroll
        for (int j = 0; j < kFqBatch; j++) {
            const double2 v = ahead[j];
            const long long nx = (long long)base0 + 64 * (kFqBatch + j) + lane;
            ahead[j] = nx < n ? nz[nx] : make_double2(0.0, 0.0);
            const double nv = sqrt(v.x * v.x + v.y * v.y);                      // fmsq.c:150
            sa[j] = scan_pole_dpp(q.onem_avm * nv, pa);
            sl[j] = scan_pole_dpp(q.onem_longavm * nv, pl);
        }
#pragma unroll
        for (int j = 0; j < kFqBatch; j++) {
            const int base = base0 + 64 * j;
            if (base >= n) break;
            const int cnt = n - base < 64 ? n - base : 64;
            const double av = sa[j] + pa.pw * avc;                               // fmsq.c:151
            const double lg = sl[j] + pl.pw * lgc;                               // fmsq.c:152
            const unsigned long long valid = cnt == 64 ? ~0ull : (1ull << cnt) - 1ull;
            const unsigned long long U = __ballot(av < q.unmute_thresh) & valid, T = __ballot(av > q.tail_thresh) & valid;
            // ready at sample i of the step when i + 1 >= wait (fmsq.c:153-154: the sample that takes ramp to tdelay is ready itself)
            const unsigned long long R = wait <= 1 ? ~0ull : wait > 64 ? 0ull : ~0ull << (wait - 1);
            avc = lane_bcast(av, cnt - 1);
            lgc = lane_bcast(lg, cnt - 1);
            wait = wait > cnt ? wait - cnt : 0;
            // nothing to do for a step that stays UNMUTED (no sample above tail_thresh): the common case on a carrier
            if (S == FQ_UNMUTED && !T) continue;
            double g = 1.0;
            bool muted = false;
            int pos = 0;
            while (pos < cnt) {
                const unsigned long long from = ~0ull << pos;
                if (S == FQ_MUTED) {                            // fmsq.c:158-166: the sample that opens is still 0
                    const unsigned long long m = U & R & from;
                    const int end = m ? __ffsll((long long)m) : cnt;
                    if (lane >= pos && lane < end) muted = true;
                    if (m) { S = FQ_INCREASE; c = q.ntup; }
                    pos = end;
                } else if (S == FQ_INCREASE || S == FQ_DECREASE) {          // fmsq.c:167-172, :194-199: count + 1 samples, count ends at -1
                    const int left = cnt - pos, len = c + 1 < left ? c + 1 : left;
                    if (lane >= pos && lane < pos + len) g = S == FQ_INCREASE ? cup[q.ntup - c + (lane - pos)] : cdown[q.ntdown - c + (lane - pos)];
                    if (c + 1 <= left) { S = S == FQ_INCREASE ? FQ_UNMUTED : FQ_MUTED; c = -1; }
                    else c -= len;
                    pos += len;
                } else if (S == FQ_UNMUTED) {                   // fmsq.c:173-182
                    const unsigned long long m = T & from;
                    if (m) {
                        const int h = __ffsll((long long)m) - 1;
                        // lnlimit in [0, 1] before the cast: a longnoise that is not a number (where the reference's cast is undefined)
                        // takes the longest tail
                        double lnlimit = lane_bcast(lg, h);
                        if (!(lnlimit <= 1.0)) lnlimit = 1.0;
                        if (lnlimit < 0.0) lnlimit = 0.0;
                        S = FQ_TAIL;
                        c = __builtin_amdgcn_readfirstlane((int)((q.min_tail + (q.max_tail - q.min_tail) * lnlimit) * q.rate));
                        pos = h + 1;
                    } else pos = cnt;
                } else {                                        // TAIL, fmsq.c:183-193: the threshold is looked at before the count
                    const unsigned long long m = U & from;
                    const int h = m ? __ffsll((long long)m) - 1 : 64;
                    const long long e = (long long)pos + c;     // the sample at which count-- finds 0
                    if (m && h <= e) { c -= h - pos; S = FQ_UNMUTED; pos = h + 1; }
                    else if (e < cnt) { S = FQ_DECREASE; c = q.ntdown; pos = (int)e + 1; }
                    else { c -= cnt - pos; pos = cnt; }
                }
            }
            if (lane < cnt) {
                if (muted) p[base + lane] = make_double2(0.0, 0.0);
                else if (g != 1.0) { const double2 z = p[base + lane]; p[base + lane] = make_double2(z.x * g, z.y * g); }
            }
        }
    }
    if (lane == 0) { FmsqState o; o.avnoise = avc; o.longnoise = lgc; o.state = S; o.count = c; o.wait = wait; state[ch] = o; }
}

// flush_fmsq (fmsq.c:122-130) for every channel (the delay lines are zeroed by the engine): not the count
static __global__ void fmsq_flush_kernel(FmsqState *state, int nch, int nready)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    state[ch].avnoise = 100.0; state[ch].longnoise = 1.0; state[ch].state = FQ_MUTED; state[ch].wait = nready;
}

}  // namespace qh
