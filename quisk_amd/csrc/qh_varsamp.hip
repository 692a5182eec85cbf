// qh_varsamp.hip -- WDSP's variable-ratio resampler VARSAMP (include/quiskhip.h group 10d): xvarsamp and its setters, wdsp/varsamp.c:29-226,
// for `nch` fp64 complex streams, every channel with its own design, varmode, run and state.
//
// The reference steps, per input sample: the sample goes into a ring of rsize; inv_cvar moves by dicvar and loses its low 16 bits; while
// isamps < 1 one output sample is made -- hshift interpolates rsize coefficients out of the R-times oversampled prototype h at h_offset,
// h_offset moves by 1 - inv_cvar and wraps into [0, 1), the coefficients meet the ring, isamps grows by inv_cvar -- and isamps drops by 1.
// Nothing in that control flow reads a sample, so the call is cut into two kernels:
//   walk     one lane per channel runs qh::varsamp_walk (qh_varsamp.hpp: the recurrence statement for statement, IEEE doubles, the bits a
//            host build gives) and leaves for every output sample m the input index i_m it is made at and the h_offset in force, the
//            channel's count, and the channel's state behind the call.  Records are laid out [m][nch]: lanes in step store side by side
//   filter   one thread per output sample, kVsTile consecutive samples of one channel a block.  The tile's input window -- from
//            i_first - (rsize - 1) to i_last, out of the call's row and, before the call, the channel's history row -- is read into
//            LDS once; every thread then forms hs[j] = h[hidx + (rsize-1-j) R] + frac (h[.. + 1] - h[..]) and adds hs[j] x[i_m - j], j = 0 ..
//            rsize - 1, the reference's order.  The lanes of a wavefront read h at nearly the same hidx (R delta apart), stride R in j.  A
//            window that does not fit the launch's LDS (rate ratios of 8 and more) is read straight from memory, same sums.
//            The last blocks of the grid's x range write the history behind the call: the last rsize - 1 inputs into the other buffer
// Channels with the same design share one copy of h (1.1 MB at R = 1024, rsize 140: once it fits an XCD's L2, 256 times it does not).
#include <algorithm>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>
#include "qh_design_bank.hpp"
#include "qh_design.hpp"
#include "qh_varsamp.hpp"

using namespace qh;

namespace {

constexpr int kVsTile = 256;                            // output samples of one channel per block
constexpr int kVsHist = 2240;                           // the largest rsize: 140 * 16 (varsamp.c:58 at a rate ratio of 16)
constexpr int kVsLdsCap = 3072;                         // complex samples of a tile's window in LDS at most (48 KB)
constexpr long long kVsMaxNcoef = 4194304;
constexpr int kVsSlots = 8;                             // calls whose var can be in flight
constexpr double kVsQ = 1.0 / 68719476736.0;            // 2^-36: what clearing 16 of 52 fraction bits can take, relative

struct VsParam {
    const double *h;
    double nom_ratio;
    int rsize, R, run, varmode;
};
static_assert(sizeof(VsParam) == 32, "the layout the kernels and the upload share");
static_assert(sizeof(VarsampState) == 32, "the layout the kernels and the upload share");

struct VsSettings {
    int in_rate, out_rate, R;
    double fc, fc_low, gain;
    int varmode, run;
};

struct VsDesign {
    int in_rate, out_rate, R;
    double fc, fc_low, gain;
    double nom_ratio;
    int rsize, ncoef;
    double *d_h = nullptr;
    ~VsDesign() { (void)hipFree(d_h); }
    bool is(const VsSettings &s) const
    {
        return in_rate == s.in_rate && out_rate == s.out_rate && R == s.R && fc == s.fc && fc_low == s.fc_low && gain == s.gain;
    }
};

// One lane per channel: the control recurrence of the call.  var: [nch], host memory the device reads.
__global__ __launch_bounds__(64) void varsamp_walk_kernel(int nch, int n, const VsParam *prm, VarsampState *state, const double *var, int *rec_i,
                                                          double *rec_h, int cap_out, int *cnt, int *user_cnt)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= nch) return;
    const VsParam p = prm[ch];
    VarsampState s = state[ch];
    int c = varsamp_walk(s, n, var[ch], p.nom_ratio, p.varmode, p.run, [&](int m, int i, double h_offset) {
        if (m < cap_out) {
            const long long at = (long long)m * nch + ch;
            rec_i[at] = i;
            rec_h[at] = h_offset;
        }
    });
    if (p.run && c > cap_out) c = cap_out;              // (the host's bound holds: never taken)
    state[ch] = s;
    cnt[ch] = c;
    if (user_cnt) user_cnt[ch] = c;
}

// Blocks 0 .. ntiles - 1 of x: kVsTile output samples of channel blockIdx.y, one a thread.  The blocks behind them: the channel's history.
__global__ __launch_bounds__(kVsTile) void varsamp_filter_kernel(const double2 *in, long long in_stride, double2 *out, long long out_stride, int n, int nch,
                                                                 const VsParam *prm, const int *cnt, const int *rec_i, const double *rec_h,
                                                                 const double2 *old_hist, double2 *new_hist, int ntiles, int lds_cap)
{
    extern __shared__ double2 s_x[];
    const int ch = blockIdx.y, tid = threadIdx.x;
    const VsParam p = prm[ch];
    const double2 *irow = in + (long long)ch * in_stride;
    const double2 *hrow = old_hist + (long long)ch * kVsHist;          // hrow[kVsHist + g]: stream sample g < 0 of the call
    if ((int)blockIdx.x >= ntiles) {
        // new_hist[kVsHist - 1 - j] <- the sample j behind the call's last one, j < rsize - 1; a channel that does not run keeps its ring
        const int j = ((int)blockIdx.x - ntiles) * kVsTile + tid;
        if (j >= p.rsize - 1) return;
        const int slot = kVsHist - 1 - j;
        const long long g = (long long)n - 1 - j;
        double2 v;
        if (!p.run) v = hrow[slot];
        else v = g >= 0 ? irow[g] : hrow[kVsHist + g];
        new_hist[(long long)ch * kVsHist + slot] = v;
        return;
    }
    const int count = cnt[ch];
    const int m0 = (int)blockIdx.x * kVsTile;
    if (m0 >= count) return;
    double2 *orow = out + (long long)ch * out_stride;
    const int m = m0 + tid;
    if (!p.run) {                                       // varsamp.c:176-177; count is n
        if (m < count) orow[m] = irow[m];
        return;
    }
    const int m1 = (m0 + kVsTile < count ? m0 + kVsTile : count) - 1;
    const int i0 = rec_i[(long long)m0 * nch + ch], i1 = rec_i[(long long)m1 * nch + ch];
    const int rsize = p.rsize, R = p.R;
    const int g0 = i0 - (rsize - 1), W = i1 - g0 + 1;   // the window: stream samples g0 .. i1
    const bool lds = W <= lds_cap;
    if (lds) {
        for (int k = tid; k < W; k += kVsTile) {
            const int g = g0 + k;
            s_x[k] = g >= 0 ? irow[g] : hrow[kVsHist + g];
        }
        __syncthreads();
    }
    if (m >= count) return;
    const int im = rec_i[(long long)m * nch + ch];
    const double pos = (double)R * rec_h[(long long)m * nch + ch];      // hshift, varsamp.c:117-119
    int hidx = (int)pos;
    const double frac = pos - (double)hidx;
    if (hidx > R - 1) hidx = R - 1;                     // (h_offset < 1: never taken; keeps the reads inside h whatever the record holds)
    if (hidx < 0) hidx = 0;
    const double *hp = p.h + ((long long)(rsize - 1) * R + hidx);       // hs[0]: the loop of varsamp.c:120 ends there
    double I = 0.0, Q = 0.0;
    if (lds) {
        const double2 *xp = s_x + (im - g0);
#pragma unroll 4
        for (int j = 0; j < rsize; j++) {
            const double a = hp[0], b = hp[1];
            const double hs = a + frac * (b - a);       // varsamp.c:121
            const double2 v = xp[-j];
            I += hs * v.x;                              // varsamp.c:164-165
            Q += hs * v.y;
            hp -= R;
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < rsize; j++) {
            const double a = hp[0], b = hp[1];
            const double hs = a + frac * (b - a);
            const int g = im - j;
            const double2 v = g >= 0 ? irow[g] : hrow[kVsHist + g];
            I += hs * v.x;
            Q += hs * v.y;
            hp -= R;
        }
    }
    orow[m] = make_double2(I, Q);
}

// flush_varsamp (varsamp.c:104-110) for channels ch0 .. ch0 + gridDim.y - 1: the ring zeroed, h_offset and isamps 0.  calc: the rest of
// calc_varsamp (varsamp.c:34-35) besides, inv_cvar from the last var and the channel's new nom_ratio
__global__ __launch_bounds__(256) void varsamp_reset_kernel(VarsampState *state, double2 *hist, const VsParam *prm, int ch0, int calc)
{
    const int ch = ch0 + blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j < kVsHist) hist[(long long)ch * kVsHist + j] = make_double2(0.0, 0.0);
    if (j == 0) {
        VarsampState &s = state[ch];
        s.h_offset = 0.0;
        s.isamps = 0.0;
        if (calc) {
            const double cvar = s.var * prm[ch].nom_ratio;
            s.inv_cvar = 1.0 / cvar;
        }
    }
}

const char *vs_refusal(const VsSettings &s)
{
    if (s.in_rate <= 0 || s.out_rate <= 0) return "the rates must be positive";
    if ((long long)s.in_rate > 16ll * s.out_rate || (long long)s.out_rate > 16ll * s.in_rate) return "the rate ratio must not exceed 16 either way";
    if (s.R < 1) return "R must be at least 1";
    int rsize;
    long long ncoef;
    varsamp_sizes(s.in_rate, s.out_rate, s.R, &rsize, &ncoef);
    if (rsize < 1 || rsize > kVsHist) return "the rate ratio must not exceed 16 either way";
    if (ncoef > kVsMaxNcoef) return "rsize * R + 1 must not exceed 4194304 coefficients";
    if (!std::isfinite(s.fc) || !std::isfinite(s.fc_low) || !std::isfinite(s.gain)) return "fc, fc_low and gain must be finite";
    return nullptr;
}

bool vs_var_ok(double v) { return std::isfinite(v) && v >= 0.5 && v <= 2.0; }

}  // namespace

int qh::varsamp_check_settings(int in_rate, int out_rate, int R, double fc, double fc_low, double gain)
{
    const char *why = vs_refusal(VsSettings{in_rate, out_rate, R, fc, fc_low, gain, 1, 1});
    return why ? set_error(QH_ERR_INVALID, "qh_varsamp_create: %s", why) : QH_OK;
}

struct qh_varsamp : DesignBank<VsSettings, VsDesign, VsParam, kVsSlots> {
    // what the host knows of every channel's inv_cvar (the value itself is in device memory): the last var and bounds of where it stands
    std::vector<double> var_last, inv_lo, inv_hi;
    VarsampState *d_state = nullptr;
    double2 *hist[2] = { nullptr, nullptr };
    int *d_cnt = nullptr;
    // per-call records, grown with the calls' bound: [cap_out][nch]
    long long cap_out = 0;
    int *d_rec_i = nullptr;
    double *d_rec_h = nullptr;
    // the calls' var: a ring of rows in host memory that the device reads, a row free again when its call's walk has run
    double *h_var = nullptr, *dv_var = nullptr;

    void free_rec()
    {
        (void)hipFree(d_rec_i); (void)hipFree(d_rec_h);
        d_rec_i = nullptr; d_rec_h = nullptr; cap_out = 0;
    }
    ~qh_varsamp()
    {
        quiesce();
        free_rec();
        (void)hipFree(d_state); (void)hipFree(hist[0]); (void)hipFree(hist[1]); (void)hipFree(d_cnt);
        if (h_var) (void)hipHostFree(h_var);
    }

    static const char *refusal(const VsSettings &s) { return vs_refusal(s); }

    // The design of `s`: one a channel of the bank (or of `more`) already has, or a new one with h in device memory.  Null: the message is set.
    std::shared_ptr<VsDesign> design(const VsSettings &s, const Designs &more, const char *name)
    {
        if (auto d = cached(s, more)) return d;
        const VarsampDesign hd = design_varsamp(s.in_rate, s.out_rate, s.R, s.fc, s.fc_low, s.gain);
        auto d = std::make_shared<VsDesign>();
        d->in_rate = s.in_rate; d->out_rate = s.out_rate; d->R = s.R; d->fc = s.fc; d->fc_low = s.fc_low; d->gain = s.gain;
        d->nom_ratio = hd.nom_ratio; d->rsize = hd.rsize; d->ncoef = hd.ncoef;
        return with_taps(d, hd.h.data(), hd.ncoef, name);
    }

    void fill_param(int ch)
    {
        const VsDesign &d = *des[ch];
        prm[ch] = VsParam{d.d_h, d.nom_ratio, d.rsize, d.R, set[ch].run, set[ch].varmode};
        dirty = true;
    }

    // design_bank_set's steps: the reset kernel reads d_prm, so the new rows go up before a restart
    int before_adopt(const Designs &, const char *) { return QH_OK; }
    void designed(int ch) { inv_known(ch, var_last[ch]); }
    int before_restart() { return upload(); }

    // inv_cvar = 1 / (var * nom_ratio) freshly set (calc_varsamp, or a call with varmode 0): its first step clears the 16 bits
    void inv_known(int ch, double var)
    {
        const double t = 1.0 / (var * des[ch]->nom_ratio);
        inv_lo[ch] = t * (1.0 - 2.0 * kVsQ);
        inv_hi[ch] = t;
    }

    // Where inv_cvar of channel ch can go during a call of n samples with `var` -> [lo, hi], and where it can stand behind it -> [elo, ehi].
    // With t = 1 / (var nom_ratio), d = (t - old) / n and q = 2^-36 every step gives (inv + d)(1 - q) <= inv' <= inv + d, so after k steps
    // inv stays above min(old, t) - k q max(old, t) and below max(old, t), and ends within n q max(old, t) below t.
    void inv_span(int ch, int n, double var, double *lo, double *hi, double *elo, double *ehi) const
    {
        const double t = 1.0 / (var * des[ch]->nom_ratio);
        if (!set[ch].varmode) {
            *lo = *elo = t * (1.0 - 2.0 * kVsQ);
            *hi = *ehi = t;
            return;
        }
        if (n == 0 || !set[ch].run) {                   // varsamp.c:136: the old value stays
            *lo = *elo = inv_lo[ch];
            *hi = *ehi = inv_hi[ch];
            return;
        }
        const double top = std::max(inv_hi[ch], t) * (1.0 + 1e-12), slack = ((double)n + 2.0) * kVsQ * top;
        *lo = std::min(inv_lo[ch], t) - slack;
        *hi = top;
        *elo = t - slack;
        *ehi = t * (1.0 + 1e-12);
    }

    // The most samples channel ch can make of n: every output adds inv_cvar >= lo to isamps, which starts at 0 or above and ends below the
    // last inv_cvar <= hi, and the n inputs take n off it
    long long bound(int ch, int n, double var) const
    {
        if (n == 0) return 0;
        if (!set[ch].run) return n;
        double lo, hi, elo, ehi;
        inv_span(ch, n, var, &lo, &hi, &elo, &ehi);
        return (long long)std::floor(((double)n + hi) / lo) + 1;
    }

    long long max_out(int n, const double *var) const
    {
        long long mo = 0;
        for (int ch = 0; ch < nch; ch++) mo = std::max(mo, bound(ch, n, var[ch]));
        return mo;
    }

    int scratch(long long mo)
    {
        if (mo <= cap_out) return QH_OK;
        QH_HIP(hipStreamSynchronize(stream));
        free_rec();
        const long long want = mo + mo / 8 + 64;
        if (dev_alloc(&d_rec_i, (size_t)want * (size_t)nch) != hipSuccess || dev_alloc(&d_rec_h, (size_t)want * (size_t)nch) != hipSuccess) {
            free_rec();
            return set_error(QH_ERR_HIP, "qh_varsamp_process: scratch allocation failed");
        }
        cap_out = want;
        return QH_OK;
    }

    int restart(int ch, int mode)                       // mode 1: flush; 2: calc_varsamp
    {
        hipLaunchKernelGGL(varsamp_reset_kernel, dim3((kVsHist + 255) / 256, 1), dim3(256), 0, stream, d_state, hist[cur], d_prm, ch, (int)(mode == 2));
        QH_HIP(hipGetLastError());
        return QH_OK;
    }
};

namespace {

const char *vs_check_call(const qh_varsamp *h, const void *in, long long in_stride, const void *out, int n, const double *var)
{
    if (!h || n < 0 || !var || (n > 0 && (!in || !out || in_stride < n))) return "bad arguments";
    for (int ch = 0; ch < h->nch; ch++)
        if (!vs_var_ok(var[ch])) return "var must be finite and lie in [0.5, 2]";
    return nullptr;
}

}  // namespace

extern "C" {

qh_varsamp *qh_varsamp_create(int device, int nch, int in_rate, int out_rate, int R, double fc, double fc_low, double gain, double var, int varmode,
                              void *stream)
{
    const VsSettings s0{in_rate, out_rate, R, fc, fc_low, gain, varmode != 0, 1};
    if (nch <= 0 || nch > 65535) { set_error(QH_ERR_INVALID, "qh_varsamp_create: bad arguments"); return nullptr; }
    if (const char *why = vs_refusal(s0)) { set_error(QH_ERR_INVALID, "qh_varsamp_create: %s", why); return nullptr; }
    if (!vs_var_ok(var)) { set_error(QH_ERR_INVALID, "qh_varsamp_create: var must be finite and lie in [0.5, 2]"); return nullptr; }
    qh_varsamp *h = new qh_varsamp();
    h->nch = nch;
    auto fail = [&](const char *what) -> qh_varsamp * { set_error(QH_ERR_HIP, "qh_varsamp_create: %s failed", what); delete h; return nullptr; };
    if (bank_open(h, device, stream, "qh_varsamp_create") != QH_OK) { delete h; return nullptr; }
    h->set.assign((size_t)nch, s0);
    h->prm.assign((size_t)nch, VsParam{});
    h->var_last.assign((size_t)nch, var);
    h->inv_lo.assign((size_t)nch, 0.0);
    h->inv_hi.assign((size_t)nch, 0.0);
    std::shared_ptr<VsDesign> d = h->design(s0, {}, "qh_varsamp_create");
    if (!d) { delete h; return nullptr; }
    h->des.assign((size_t)nch, d);
    const double cvar = var * d->nom_ratio;             // varsamp.c:34-35
    std::vector<VarsampState> st((size_t)nch, VarsampState{1.0 / cvar, 0.0, 0.0, var});
    for (int ch = 0; ch < nch; ch++) { h->fill_param(ch); h->inv_known(ch, var); }
    const size_t hb = (size_t)nch * kVsHist;
    if (dev_alloc(&h->d_prm, (size_t)nch) != hipSuccess || dev_alloc(&h->d_state, (size_t)nch) != hipSuccess || dev_alloc(&h->d_cnt, (size_t)nch) != hipSuccess ||
        dev_alloc(&h->hist[0], hb) != hipSuccess || dev_alloc(&h->hist[1], hb) != hipSuccess)
        return fail("hipMalloc");
    if (hipHostMalloc((void **)&h->h_var, (size_t)kVsSlots * (size_t)nch * sizeof(double), hipHostMallocDefault) != hipSuccess) { h->h_var = nullptr; return fail("hipHostMalloc"); }
    if (hipHostGetDevicePointer((void **)&h->dv_var, h->h_var, 0) != hipSuccess) return fail("hipHostGetDevicePointer");
    if (!h->create_slots()) return fail("event creation");
    // the ring of the reference is zeroed (malloc0, varsamp.c:63)
    if (dev_zero(h->hist[0], hb * sizeof(double2)) != hipSuccess || dev_zero(h->hist[1], hb * sizeof(double2)) != hipSuccess ||
        dev_zero(h->d_cnt, (size_t)nch * sizeof(int)) != hipSuccess)
        return fail("hipMemset");
    if (hipMemcpy(h->d_state, st.data(), (size_t)nch * sizeof(VarsampState), hipMemcpyHostToDevice) != hipSuccess) return fail("hipMemcpy");
    if (h->upload() != QH_OK) { delete h; return nullptr; }
    return h;
}

void qh_varsamp_destroy(qh_varsamp *h) { delete h; }

int qh_varsamp_rsize(qh_varsamp *h, int ch)
{
    if (!h || ch < 0 || ch >= h->nch) return 0;
    std::lock_guard<std::mutex> lk(h->mtx);
    return h->des[ch]->rsize;
}

int qh_varsamp_flush(qh_varsamp *h, int ch) { return design_bank_set(h, ch, "qh_varsamp_flush", 1, [](VsSettings &) { return true; }); }
int qh_varsamp_set_run(qh_varsamp *h, int ch, int run) { return design_bank_set(h, ch, "qh_varsamp_set_run", 0, [=](VsSettings &s) { s.run = run != 0; return true; }); }
int qh_varsamp_set_varmode(qh_varsamp *h, int ch, int varmode)
{
    return design_bank_set(h, ch, "qh_varsamp_set_varmode", 0, [=](VsSettings &s) { s.varmode = varmode != 0; return true; });
}
int qh_varsamp_set_rates(qh_varsamp *h, int ch, int in_rate, int out_rate)
{
    return design_bank_set(h, ch, "qh_varsamp_set_rates", 2, [=](VsSettings &s) { s.in_rate = in_rate; s.out_rate = out_rate; return true; });
}
int qh_varsamp_set_bandwidth(qh_varsamp *h, int ch, double fc_low, double fc_high)
{
    return design_bank_set(h, ch, "qh_varsamp_set_bandwidth", 2, [=](VsSettings &s) {
        if (fc_low == s.fc_low && fc_high == s.fc) return false;        // varsamp.c:219
        s.fc_low = fc_low; s.fc = fc_high;
        return true;
    });
}

long long qh_varsamp_max_out(qh_varsamp *h, int n, const double *var)
{
    if (const char *why = vs_check_call(h, nullptr, 0, nullptr, n > 0 ? 0 : n, var)) return set_error(QH_ERR_INVALID, "qh_varsamp_max_out: %s", why);
    std::lock_guard<std::mutex> lk(h->mtx);
    return h->max_out(n, var);
}

int qh_varsamp_process(qh_varsamp *h, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n, const double *var, int *d_count)
{
    if (const char *why = vs_check_call(h, d_in, in_stride, d_out, n, var)) return set_error(QH_ERR_INVALID, "qh_varsamp_process: %s", why);
    std::lock_guard<std::mutex> lk(h->mtx);
    const long long mo = h->max_out(n, var);
    if (n > 0 && out_stride < mo) return set_error(QH_ERR_INVALID, "qh_varsamp_process: out_stride %lld is below qh_varsamp_max_out = %lld", out_stride, mo);
    if (rows_overlap(d_in, in_stride * 16, (long long)n * 16, d_out, out_stride * 16, mo * 16, h->nch))
        return set_error(QH_ERR_INVALID, "qh_varsamp_process: the output rows overlap the input rows (an output is a sum over the inputs around it)");
    QH_HIP(hipSetDevice(h->device));
    if (int rc = h->upload()) return rc;
    if (int rc = h->scratch(mo)) return rc;
    const int nch = h->nch;
    hipStream_t s = h->stream;
    int sl;
    if (int rc = h->take_slot(&sl)) return rc;
    std::copy(var, var + nch, h->h_var + (size_t)sl * nch);
    hipLaunchKernelGGL(varsamp_walk_kernel, dim3((unsigned)((nch + 63) / 64)), dim3(64), 0, s, nch, n, h->d_prm, h->d_state, h->dv_var + (size_t)sl * nch,
                       h->d_rec_i, h->d_rec_h, (int)std::min<long long>(h->cap_out, 0x7fffffff), h->d_cnt, d_count);
    QH_HIP(hipGetLastError());
    if (int rc = h->slot_enqueued()) return rc;
    // the window a tile of a running channel can need, for the launch's LDS
    long long need = 1;
    int hist_rows = 0;
    for (int ch = 0; ch < nch; ch++) {
        double lo, hi, elo, ehi;
        h->inv_span(ch, n, var[ch], &lo, &hi, &elo, &ehi);
        if (h->set[ch].run && n > 0) need = std::max(need, (long long)h->des[ch]->rsize + (long long)std::ceil(kVsTile * hi) + 2);
        hist_rows = std::max(hist_rows, h->des[ch]->rsize - 1);
        h->var_last[ch] = var[ch];
        h->inv_lo[ch] = elo;
        h->inv_hi[ch] = ehi;
    }
    if (n == 0) return QH_OK;
    const int lds_cap = (int)std::min<long long>(need, kVsLdsCap);
    const int ntiles = (int)((mo + kVsTile - 1) / kVsTile), nhb = (hist_rows + kVsTile - 1) / kVsTile;
    hipLaunchKernelGGL(varsamp_filter_kernel, dim3((unsigned)(ntiles + nhb), (unsigned)nch), dim3(kVsTile), (size_t)lds_cap * sizeof(double2), s,
                       static_cast<const double2 *>(d_in), in_stride, static_cast<double2 *>(d_out), out_stride, n, nch, h->d_prm, h->d_cnt, h->d_rec_i,
                       h->d_rec_h, h->hist[h->cur], h->hist[h->cur ^ 1], ntiles, lds_cap);
    QH_HIP(hipGetLastError());
    h->cur ^= 1;
    return QH_OK;
}

int qh_varsamp_process_host(qh_varsamp *h, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n, const double *var, int *h_count)
{
    if (const char *why = vs_check_call(h, h_in, in_stride, h_out, n, var)) return set_error(QH_ERR_INVALID, "qh_varsamp_process_host: %s", why);
    if (!h_count) return set_error(QH_ERR_INVALID, "qh_varsamp_process_host: bad arguments");
    const long long mo = qh_varsamp_max_out(h, n, var);
    if (mo < 0) return (int)mo;
    if (n > 0 && out_stride < mo) return set_error(QH_ERR_INVALID, "qh_varsamp_process_host: out_stride %lld is below qh_varsamp_max_out = %lld", out_stride, mo);
    QH_HIP(hipSetDevice(h->device));
    const size_t nch = (size_t)h->nch;
    double2 *d = nullptr, *o = nullptr;
    int *c = nullptr;
    int rc = QH_OK;
    if (hipMalloc((void **)&d, std::max<size_t>(nch * (size_t)n, 1) * sizeof(double2)) != hipSuccess ||
        hipMalloc((void **)&o, std::max<size_t>(nch * (size_t)mo, 1) * sizeof(double2)) != hipSuccess || hipMalloc((void **)&c, nch * sizeof(int)) != hipSuccess)
        rc = set_error(QH_ERR_HIP, "qh_varsamp_process_host: hipMalloc failed");
    if (rc == QH_OK && n > 0 &&
        hipMemcpy2DAsync(d, (size_t)n * 16, h_in, (size_t)in_stride * 16, (size_t)n * 16, nch, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        rc = set_error(QH_ERR_HIP, "qh_varsamp_process_host: upload failed");
    if (rc == QH_OK) rc = qh_varsamp_process(h, d, n, o, mo, n, var, c);
    if (rc == QH_OK && (hipMemcpyAsync(h_count, c, nch * sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess))
        rc = set_error(QH_ERR_HIP, "qh_varsamp_process_host: download failed");
    // nothing behind a row's count: one copy where the counts agree, else row by row
    if (rc == QH_OK && n > 0) {
        bool same = true;
        for (size_t ch = 1; ch < nch; ch++) same = same && h_count[ch] == h_count[0];
        hipError_t e = hipSuccess;
        if (same && h_count[0] > 0)
            e = hipMemcpy2DAsync(h_out, (size_t)out_stride * 16, o, (size_t)mo * 16, (size_t)h_count[0] * 16, nch, hipMemcpyDeviceToHost, h->stream);
        else if (!same)
            for (size_t ch = 0; ch < nch && e == hipSuccess; ch++)
                if (h_count[ch] > 0)
                    e = hipMemcpyAsync(static_cast<double2 *>(h_out) + ch * (size_t)out_stride, o + ch * (size_t)mo, (size_t)h_count[ch] * 16,
                                       hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) rc = set_error(QH_ERR_HIP, "qh_varsamp_process_host: download failed");
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == QH_OK) rc = set_error(QH_ERR_HIP, "qh_varsamp_process_host: synchronize failed");
    (void)hipFree(d); (void)hipFree(o); (void)hipFree(c);
    return rc;
}

int qh_varsamp_synchronize(qh_varsamp *h) { return bank_synchronize(h, "qh_varsamp_synchronize"); }

}  // extern "C"
