// qh_anb.hip -- WDSP's noise blanker ANB (include/quiskhip.h group 10b): xanb and its setters, wdsp/nob.c:33-187,348-422, for `nch`
// fp64 complex streams at the receiver's input rate, every channel with its own settings and state.
//
// The reference steps, per sample: mag = |x|; avg = backmult avg + (1 - backmult) mag; a trigger (mag > avg threshold) loads `count`
// with T = trans_count + adv_count; a five-state machine looks at count (pass / cosine fall / dead time / hang / cosine rise) and
// scales the sample T behind the newest one; count drops by one.  So the machine sees count > 0 at sample i exactly when a trigger
// lies in (i - T, i], and the call is cut into passes:
//   det 0 / carry / det 1    the detector of qh_blank_det.hpp: the trigger bits, 64 samples a word              (two reads of the rows)
//   walk     one wavefront per channel, 64 words at a time: the trigger bits dilated by T (the "count > 0" bits, kept for the apply
//            pass), then the machine from event to event -- the next set / clear bit by __ballot and a bit scan, a ramp, the dead
//            time and a quiet hang skipped whole.  It leaves (state, timer, power, htime) at every word's first sample and the
//            channel's state behind the call
//   apply    one thread per output sample, one wavefront per word: the word's record and its count bits give every lane its
//            segment (event by event, uniform over the wavefront); the sample i - T comes from the call's rows or from the history
//            of the last kAnbHist input samples; copy, zeros or the reference's product                 (one read, one write)
//   hist     the last kAnbHist input samples of every running channel to the other history buffer
// Given the trigger bits (see the header for where they can differ from a sample-serial run), the output is the reference's bit for
// bit: wave[], backmult and the counts are computed on the host with the C library the reference calls, and the two products of a
// scaled sample are the reference's.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>
#include "qh_blank_det.hpp"

using namespace qh;

namespace {

constexpr double kAnbMaxTau = 0.002, kAnbMaxAdv = 0.002, kAnbMaxRate = 1536000.0;      // nob.c:29-31
constexpr int kAnbMaxTrans = 3072;                      // (int)(MAX_SAMPLERATE * MAX_TAU), nob.c:80
constexpr int kAnbWave = kAnbMaxTrans + 1;              // doubles of wave[] per channel
constexpr int kAnbHist = 2 * kAnbMaxTrans;              // the longest delay, nob.c:81

struct AnbParam {
    double backmult, ombackmult, threshold;
    double carry;                       // backmult^kDetL
    int tc, adv, hang, T;               // trans_count, adv_count, hang_count, tc + adv
    int run, pad;
};
static_assert(sizeof(AnbParam) == 56, "the layout the kernels and the upload share");

// what xanb keeps from call to call, but for the delay line (hist).  timer: dtime, atime or itime, whichever the state counts
struct AnbState {
    double avg, power;
    int state, timer, htime, count;
};
static_assert(sizeof(AnbState) == 32, "the layout the kernels share");

struct AnbRec {                         // the machine at a word's first sample: st = state | timer << 3
    double power;
    int st, htime;
};

// bit k of the result: word sample ws + k lies in [lo, hi)
__device__ __forceinline__ u64 anb_range(long long ws, long long lo, long long hi)
{
    long long a = lo - ws, b = hi - ws;
    a = a < 0 ? 0 : a > 64 ? 64 : a;
    b = b < 0 ? 0 : b > 64 ? 64 : b;
    if (a >= b) return 0ull;
    const u64 top = b == 64 ? ~0ull : (1ull << b) - 1ull;
    return top & ~((1ull << a) - 1ull);
}

// the first set bit of `bits` at or after `from`, 64 if none
__device__ __forceinline__ int anb_first(u64 bits, int from)
{
    const u64 m = from >= 64 ? 0ull : bits & (~0ull << from);
    return m ? __ffsll((long long)m) - 1 : 64;
}

// The event walk, one wavefront per channel, 64 words (4096 samples) at a time; lane l holds word l.  cb: the "count > 0" bits.
__global__ __launch_bounds__(64) void anb_walk_kernel(int n, const AnbParam *prm, AnbState *state, const double *wave, const u64 *trb, u64 *cb,
                                                      AnbRec *rec, long long wstride)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    const AnbParam p = prm[ch];
    if (!p.run) return;
    AnbState *st = state + ch;
    const double *wv = wave + (long long)ch * kAnbWave;
    const int T = p.T, tc = p.tc, adv = p.adv, hang = p.hang;
    int S = st->state, tm = st->timer, h = st->htime;
    double pw = st->power;
    long long lt = (long long)st->count - T;            // the last trigger so far, relative to the call's first sample
    const u64 *t = trb + (long long)ch * wstride;
    u64 *c = cb + (long long)ch * wstride;
    AnbRec *r = rec + (long long)ch * wstride;
    const long long nw = ((long long)n + 63) / 64;
    for (long long c0 = 0; c0 < nw; c0 += 64) {
        const long long wi = c0 + lane, ws = wi * 64, cs = c0 * 64, ce = cs + 4096 < n ? cs + 4096 : (long long)n;
        const u64 tw = wi < nw ? t[wi] : 0ull;
        // the last trigger before each word: a running maximum over the lanes, behind the chunks before
        long long inc = tw ? ws + 63 - __clzll((long long)tw) : LLONG_MIN / 2;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(inc, d, 64);
            if (lane >= d && up > inc) inc = up;
        }
        const long long ex = __shfl_up(inc, 1, 64);
        const long long ltb = lane && ex > lt ? ex : lt;
        u64 cbw = dilate(tw, T);
        const long long left = (long long)T - (ws - ltb);                   // samples of the word a trigger before it still covers
        if (left > 0) cbw |= left >= 64 ? ~0ull : (1ull << left) - 1ull;
        cbw &= anb_range(ws, cs, ce);
        if (wi < nw) c[wi] = cbw;
        const long long top = __shfl(inc, 63, 64);
        if (top > lt) lt = top;
        // the first sample in [from, to) whose bit is set in the lanes' `bits`, `to` if none
        auto find = [&](u64 bits, long long from, long long to) -> long long {
            const u64 m = bits & anb_range(ws, from, to);
            const u64 bal = __ballot(m != 0ull);
            if (!bal) return to;
            const int l0 = __ffsll((long long)bal) - 1;
            const u64 ml = __shfl(m, l0, 64);
            return (c0 + l0) * 64 + __ffsll((long long)ml) - 1;
        };
        AnbRec mine{1.0, 0, 0};
        auto note = [&](long long lo, long long hi, int stv, int hv) {      // samples lo .. hi are one segment of the machine
            if (ws >= lo && ws <= hi && ws < ce) { mine.power = pw; mine.st = stv; mine.htime = hv; }
        };
        long long pp = cs;
        while (pp < ce) {
            if (S == 0) {                                                   // nob.c:127-136
                const long long hit = find(cbw, pp, ce);
                note(pp, hit, 0, h);
                if (hit >= ce) break;
                S = 1; tm = 0; pw = 1.0; pp = hit + 1;
            } else if (S == 1 || S == 2) {                                  // nob.c:137-152: the fall, the dead time
                const long long end = pp + ((S == 1 ? tc : adv) - tm);
                note(pp, end, S | ((tm + (int)(ws - pp)) << 3), h);
                if (end < ce) { S = S == 1 ? 2 : 3; tm = 0; pp = end + 1; }
                else { tm += (int)(ce - pp); pp = ce; }
            } else if (S == 3) {                                            // nob.c:153-164
                const long long hit = find(cbw, pp, ce);
                if (hit == pp) {                                            // count > 0: htime = 1 - count up to the run's last sample
                    const long long q = find(~cbw, pp, ce);
                    note(pp, q - 1, 3, h);
                    h = q < ce ? 0 : 1 - (int)((long long)T - (ce - 1 - lt));
                    pp = q;
                } else {
                    long long m = (long long)hang - h + 1;                  // quiet samples until ++htime > hang_count
                    if (m < 1) m = 1;
                    if (hit < ce && hit < pp + m) { note(pp, hit - 1, 3, h + (int)(ws - pp)); h += (int)(hit - pp); pp = hit; }
                    else if (pp + m <= ce) { note(pp, pp + m - 1, 3, h + (int)(ws - pp)); h += (int)m; S = 4; tm = 0; pp += m; }
                    else { note(pp, ce - 1, 3, h + (int)(ws - pp)); h += (int)(ce - pp); pp = ce; }
                }
            } else {                                                        // nob.c:165-177: the rise, a trigger restarts the fall
                const long long end = pp + (tc - tm), lim = end + 1 < ce ? end + 1 : ce;
                const long long hit = find(cbw, pp, lim);
                note(pp, hit < lim ? hit : end, 4 | ((tm + (int)(ws - pp)) << 3), h);
                if (hit < lim) { pw = 0.5 - wv[tm + (int)(hit - pp)]; S = 1; tm = 0; pp = hit + 1; }
                else if (end < ce) { S = 0; tm = 0; pp = end + 1; }
                else { tm += (int)(ce - pp); pp = ce; }
            }
        }
        if (wi < nw) r[wi] = mine;
    }
    if (lane == 0) {
        const long long cnt = (long long)T - ((long long)n - lt);
        st->state = S; st->timer = tm; st->htime = h; st->power = pw;
        st->count = cnt > 0 ? (int)cnt : 0;
    }
}

// One thread per output sample, one wavefront per word.  A channel with run = 0 copies (nob.c:185-186).
__global__ __launch_bounds__(256) void anb_apply_kernel(const double2 *in, long long in_stride, double2 *out, long long out_stride, int n,
                                                        const AnbParam *prm, const double2 *hist, const double *wave, const u64 *cb,
                                                        const AnbRec *rec, long long wstride)
{
    const int ch = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, wi = i >> 6;
    if (wi * 64 >= n) return;
    const double2 *irow = in + (long long)ch * in_stride;
    double2 *orow = out + (long long)ch * out_stride;
    if (!prm[ch].run) {
        if (i < n) orow[i] = irow[i];
        return;
    }
    const int k = (int)(i & 63), tc = prm[ch].tc, adv = prm[ch].adv, hang = prm[ch].hang, T = prm[ch].T;
    const AnbRec r = rec[(long long)ch * wstride + wi];
    const u64 cbw = cb[(long long)ch * wstride + wi];
    const double *wv = wave + (long long)ch * kAnbWave;
    int S = r.st & 7, tm = r.st >> 3, h = r.htime;
    double pw = r.power, scale = 1.0;
    int kind = 0;                                       // 0 copy, 1 zeros, 2 times scale
    for (int pos = 0; pos < 64 && (S != 0 || (cbw >> pos) != 0ull);) {
        if (S == 0) {
            const int f = anb_first(cbw, pos);          // < 64 here
            if (k >= pos && k <= f) kind = 0;
            S = 1; tm = 0; pw = 1.0; pos = f + 1;
        } else if (S == 1) {
            const int end = pos + (tc - tm);
            if (k >= pos && k <= end) { kind = 2; scale = pw * (0.5 + wv[tm + k - pos]); }      // nob.c:138
            S = 2; tm = 0; pos = end + 1;
        } else if (S == 2) {
            const int end = pos + (adv - tm);
            if (k >= pos && k <= end) kind = 1;
            S = 3; pos = end + 1;
        } else if (S == 3) {
            if ((cbw >> pos) & 1ull) {
                const int q = anb_first(~cbw, pos);
                if (k >= pos && k < q) kind = 1;
                h = 0; pos = q;
            } else {
                long long m = (long long)hang - h + 1;
                if (m < 1) m = 1;
                const int f = anb_first(cbw, pos);
                if (f < 64 && f < pos + m) {
                    if (k >= pos && k < f) kind = 1;
                    pos = f;
                } else {
                    if (k >= pos && k < pos + m) kind = 1;
                    if (pos + m >= 64) break;
                    h += (int)m; S = 4; tm = 0; pos += (int)m;
                }
            }
        } else {
            const int end = pos + (tc - tm), f = anb_first(cbw, pos);
            if (f < 64 && f <= end) {
                if (k >= pos && k <= f) { kind = 2; scale = 0.5 - wv[tm + k - pos]; }           // nob.c:166
                pw = 0.5 - wv[tm + f - pos];
                S = 1; tm = 0; pos = f + 1;
            } else {
                if (k >= pos && k <= end) { kind = 2; scale = 0.5 - wv[tm + k - pos]; }
                S = 0; pos = end + 1;
            }
        }
    }
    if (i >= n) return;
    if (kind == 1) { orow[i] = make_double2(0.0, 0.0); return; }
    double2 v = i >= T ? irow[i - T] : hist[(long long)ch * kAnbHist + (kAnbHist + (i - T))];
    if (kind == 2) { v.x = v.x * scale; v.y = v.y * scale; }
    orow[i] = v;
}

// new_hist[j] <- stream sample n - kAnbHist + j of a running channel; a channel that does not run keeps its delay line
__global__ __launch_bounds__(256) void anb_hist_kernel(const double2 *in, long long in_stride, int n, const AnbParam *prm, const double2 *old_hist,
                                                       double2 *new_hist)
{
    const int ch = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= kAnbHist) return;
    const long long g = (long long)n - kAnbHist + j, row = (long long)ch * kAnbHist;
    double2 v;
    if (!prm[ch].run) v = old_hist[row + j];
    else v = g >= 0 ? in[(long long)ch * in_stride + g] : old_hist[row + (kAnbHist + g)];
    new_hist[row + j] = v;
}

// initBlanker (nob.c:33-52) for channels ch0 .. ch0 + gridDim.y - 1: the detector and the machine start over, the delay line is
// zeroed; htime and the timers are left as they are
__global__ __launch_bounds__(256) void anb_reset_kernel(AnbState *state, double2 *hist, int ch0)
{
    const int ch = ch0 + blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j < kAnbHist) hist[(long long)ch * kAnbHist + j] = make_double2(0.0, 0.0);
    if (j == 0) { AnbState &s = state[ch]; s.avg = 1.0; s.power = 1.0; s.state = 0; s.count = 0; }
}

struct AnbSettings {
    double samplerate, tau, hangtime, advtime, backtau, threshold;
    int run;
};

const char *anb_refusal(const AnbSettings &s)
{
    if (!(s.samplerate > 0.0 && s.samplerate <= kAnbMaxRate)) return "the sample rate must lie in (0, 1536000]";
    if (!(s.tau >= 0.0 && s.tau <= kAnbMaxTau)) return "tau must lie in [0, 0.002]";
    if (!(s.advtime >= 0.0 && s.advtime <= kAnbMaxAdv)) return "advtime must lie in [0, 0.002]";
    if (!(s.backtau > 0.0) || !std::isfinite(s.backtau)) return "backtau must be finite and positive";
    if (!std::isfinite(s.threshold)) return "the threshold must be finite";
    if (!(s.hangtime >= 0.0)) return "hangtime must not be negative";
    if (!(s.hangtime * s.samplerate < 1073741824.0)) return "hangtime times the sample rate must stay below 2^30 samples";
    return nullptr;
}

}  // namespace

int qh::anb_check_settings(double samplerate, double tau, double hangtime, double advtime, double backtau, double threshold)
{
    const char *why = anb_refusal(AnbSettings{samplerate, tau, hangtime, advtime, backtau, threshold, 1});
    return why ? set_error(QH_ERR_INVALID, "qh_anb_create: %s", why) : QH_OK;       // (the text create_anbEXT has always reported)
}

struct qh_anb : DetBank {
    std::vector<AnbSettings> set;
    std::vector<AnbParam> prm;
    std::vector<double> wave;                           // [nch][kAnbWave]
    std::vector<char> wave_dirty;
    AnbParam *d_prm = nullptr;
    AnbState *d_state = nullptr;
    double *d_wave = nullptr;
    double2 *hist[2] = { nullptr, nullptr };
    // per-call scratch beside the detector's, grown with it
    u64 *d_cb = nullptr;
    AnbRec *d_rec = nullptr;
    void free_walk()
    {
        (void)hipFree(d_cb); (void)hipFree(d_rec);
        d_cb = nullptr; d_rec = nullptr;
    }
    ~qh_anb()
    {
        quiesce();
        free_walk();
        (void)hipFree(d_prm); (void)hipFree(d_state); (void)hipFree(d_wave); (void)hipFree(hist[0]); (void)hipFree(hist[1]);
    }

    static const char *refusal(const AnbSettings &s) { return anb_refusal(s); }

    // initBlanker's numbers (nob.c:36-50), with the C library's exp and cos
    void derive(int ch)
    {
        const AnbSettings &s = set[ch];
        AnbParam &p = prm[ch];
        p.tc = (int)(s.tau * s.samplerate);
        if (p.tc < 2) p.tc = 2;
        p.hang = (int)(s.hangtime * s.samplerate);
        p.adv = (int)(s.advtime * s.samplerate);
        p.T = p.tc + p.adv;
        const double coef = 3.1415926535897932 / p.tc;      // PI, comm.h
        p.backmult = std::exp(-1.0 / (s.samplerate * s.backtau));
        p.ombackmult = 1.0 - p.backmult;
        p.carry = std::pow(p.backmult, (double)kDetL);
        p.threshold = s.threshold;
        p.run = s.run;
        p.pad = 0;
        double *w = wave.data() + (size_t)ch * kAnbWave;
        for (int i = 0; i <= p.tc; i++) w[i] = 0.5 * std::cos(i * coef);
        wave_dirty[ch] = 1;
        dirty = true;
    }

    void apply_light(int ch) { prm[ch].threshold = set[ch].threshold; prm[ch].run = set[ch].run; }

    int restart(int ch0, int count)
    {
        hipLaunchKernelGGL(anb_reset_kernel, dim3((kAnbHist + 255) / 256, (unsigned)count), dim3(256), 0, stream, d_state, hist[cur], ch0);
        QH_HIP(hipGetLastError());
        return QH_OK;
    }

    // host settings -> device, behind everything enqueued so far (the copies are synchronous: the vectors may change right after)
    int upload()
    {
        if (!dirty) return QH_OK;
        QH_HIP(hipStreamSynchronize(stream));
        QH_HIP(hipMemcpy(d_prm, prm.data(), (size_t)nch * sizeof(AnbParam), hipMemcpyHostToDevice));
        for (int ch = 0; ch < nch; ch++) {
            if (!wave_dirty[ch]) continue;
            QH_HIP(hipMemcpy(d_wave + (size_t)ch * kAnbWave, wave.data() + (size_t)ch * kAnbWave, (size_t)(prm[ch].tc + 1) * sizeof(double),
                             hipMemcpyHostToDevice));
            wave_dirty[ch] = 0;
        }
        dirty = false;
        return QH_OK;
    }

    int scratch(int n)
    {
        if (n <= cap) return QH_OK;
        if (int rc = bank_grow(this, n, kDetL, "qh_anb_process")) return rc;
        free_walk();
        if (dev_alloc(&d_cb, (size_t)nch * (size_t)nw) != hipSuccess || dev_alloc(&d_rec, (size_t)nch * (size_t)nw) != hipSuccess) {
            free_walk();
            free_scratch();
            return set_error(QH_ERR_HIP, "qh_anb_process: scratch allocation failed");
        }
        return QH_OK;
    }
};

extern "C" {

qh_anb *qh_anb_create(int device, int nch, double samplerate, double tau, double hangtime, double advtime, double backtau, double threshold,
                      void *stream)
{
    const AnbSettings s0{samplerate, tau, hangtime, advtime, backtau, threshold, 1};
    if (nch <= 0) { set_error(QH_ERR_INVALID, "qh_anb_create: bad arguments"); return nullptr; }
    if (const char *why = anb_refusal(s0)) { set_error(QH_ERR_INVALID, "qh_anb_create: %s", why); return nullptr; }
    qh_anb *h = new qh_anb();
    h->nch = nch;
    auto fail = [&](const char *what) -> qh_anb * { set_error(QH_ERR_HIP, "qh_anb_create: %s failed", what); delete h; return nullptr; };
    if (bank_open(h, device, stream, "qh_anb_create") != QH_OK) { delete h; return nullptr; }
    h->set.assign((size_t)nch, s0);
    h->prm.assign((size_t)nch, AnbParam{});
    h->wave.assign((size_t)nch * kAnbWave, 0.0);
    h->wave_dirty.assign((size_t)nch, 1);
    h->derive(0);
    for (int ch = 1; ch < nch; ch++) {
        h->prm[ch] = h->prm[0];
        std::copy(h->wave.begin(), h->wave.begin() + kAnbWave, h->wave.begin() + (size_t)ch * kAnbWave);
    }
    const size_t hb = (size_t)nch * kAnbHist;
    if (dev_alloc(&h->d_prm, (size_t)nch) != hipSuccess || dev_alloc(&h->d_state, (size_t)nch) != hipSuccess ||
        dev_alloc(&h->d_wave, (size_t)nch * kAnbWave) != hipSuccess || dev_alloc(&h->hist[0], hb) != hipSuccess ||
        dev_alloc(&h->hist[1], hb) != hipSuccess)
        return fail("hipMalloc");
    // the allocation of the reference is zeroed (malloc0, nob.c:69): htime and the timers start at 0
    if (dev_zero(h->d_state, (size_t)nch * sizeof(AnbState)) != hipSuccess || dev_zero(h->d_wave, (size_t)nch * kAnbWave * sizeof(double)) != hipSuccess ||
        dev_zero(h->hist[1], hb * sizeof(double2)) != hipSuccess)
        return fail("hipMemset");
    if (h->restart(0, nch) != QH_OK) { delete h; return nullptr; }
    return h;
}

void qh_anb_destroy(qh_anb *h) { delete h; }

int qh_anb_delay(qh_anb *h, int ch)
{
    if (!h || ch < 0 || ch >= h->nch) return 0;
    std::lock_guard<std::mutex> lk(h->mtx);
    return h->prm[ch].T;
}

int qh_anb_set_run(qh_anb *h, int ch, int run) { return bank_set(h, ch, "qh_anb_set_run", false, [=](AnbSettings &s) { s.run = run != 0; }); }
int qh_anb_set_samplerate(qh_anb *h, int ch, double samplerate) { return bank_set(h, ch, "qh_anb_set_samplerate", true, [=](AnbSettings &s) { s.samplerate = samplerate; }); }
int qh_anb_set_tau(qh_anb *h, int ch, double tau) { return bank_set(h, ch, "qh_anb_set_tau", true, [=](AnbSettings &s) { s.tau = tau; }); }
int qh_anb_set_hangtime(qh_anb *h, int ch, double hangtime) { return bank_set(h, ch, "qh_anb_set_hangtime", true, [=](AnbSettings &s) { s.hangtime = hangtime; }); }
int qh_anb_set_advtime(qh_anb *h, int ch, double advtime) { return bank_set(h, ch, "qh_anb_set_advtime", true, [=](AnbSettings &s) { s.advtime = advtime; }); }
int qh_anb_set_backtau(qh_anb *h, int ch, double backtau) { return bank_set(h, ch, "qh_anb_set_backtau", true, [=](AnbSettings &s) { s.backtau = backtau; }); }
int qh_anb_set_threshold(qh_anb *h, int ch, double threshold) { return bank_set(h, ch, "qh_anb_set_threshold", false, [=](AnbSettings &s) { s.threshold = threshold; }); }
int qh_anb_flush(qh_anb *h, int ch) { return bank_set(h, ch, "qh_anb_flush", true, [](AnbSettings &) {}); }

int qh_anb_process(qh_anb *h, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n)
{
    if (int rc = bank_check_rows("qh_anb_process", h, d_in, in_stride, d_out, out_stride, n, "an output is the input T samples back")) return rc;
    if (n == 0) return QH_OK;
    std::lock_guard<std::mutex> lk(h->mtx);
    QH_HIP(hipSetDevice(h->device));
    if (int rc = h->upload()) return rc;
    if (int rc = h->scratch(n)) return rc;
    const double2 *in = static_cast<const double2 *>(d_in);
    double2 *out = static_cast<double2 *>(d_out);
    const long long nw = h->nw;
    const unsigned nch = (unsigned)h->nch;
    bool any = false;
    for (const AnbParam &p : h->prm) any = any || p.run;
    hipStream_t s = h->stream;
    if (any) {
        det_enqueue(*h, in, in_stride, n, h->d_prm, h->d_state);
        hipLaunchKernelGGL(anb_walk_kernel, dim3(nch), dim3(64), 0, s, n, h->d_prm, h->d_state, h->d_wave, h->d_trb, h->d_cb, h->d_rec, nw);
    }
    hipLaunchKernelGGL(anb_apply_kernel, dim3((unsigned)((n + 255) / 256), nch), dim3(256), 0, s, in, in_stride, out, out_stride, n, h->d_prm,
                       h->hist[h->cur], h->d_wave, h->d_cb, h->d_rec, nw);
    if (any) {
        hipLaunchKernelGGL(anb_hist_kernel, dim3((kAnbHist + 255) / 256, nch), dim3(256), 0, s, in, in_stride, n, h->d_prm, h->hist[h->cur],
                           h->hist[h->cur ^ 1]);
        h->cur ^= 1;
    }
    QH_HIP(hipGetLastError());
    return QH_OK;
}

int qh_anb_process_host(qh_anb *h, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n)
{
    return bank_process_host(h, h_in, in_stride, h_out, out_stride, n, qh_anb_process, "qh_anb_process_host");
}

int qh_anb_synchronize(qh_anb *h) { return bank_synchronize(h, "qh_anb_synchronize"); }

}  // extern "C"
