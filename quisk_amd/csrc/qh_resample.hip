// qh_resample.hip -- WDSP's fixed-ratio resampler RESAMPLE / RESAMPLEF (include/quiskhip.h group 10f): xresample, xresampleF and their
// setters, wdsp/resample.c:35-204,236-330, for `nch` streams of fp64 complex or fp32 real samples, every channel with its own design, run
// and state.
//
// The reference steps, per input sample: the sample goes into a ring of cpp; while phnum < L one output is made from tap row phnum of
// the phase-major h[L][cpp] against the ring, newest sample first, and phnum moves by M; then phnum drops by L.  So output m of a call
// sits at upsampled position p = phnum + m M, is made at input p / L with row p % L, and a call of n samples makes
// ceil((n L - phnum) / M) of them: count and next phnum are a closed form the host evaluates, and every output can be made on its own.
//
// One kernel a call.  A block takes a tile of one channel's outputs in which every tap row is used by G outputs (G a power of two): the
// tile is G L consecutive outputs, the G outputs of row r lie L apart and their inputs M apart.  Lanes are laid over (row, g) with g
// fastest, so the G lanes of a row read one tap address (a wavefront of one row -- G >= 64 -- takes its taps as scalar loads and keeps
// the whole address walk in scalar registers) and the vector unit does the multiply-adds.  The tile's input window (about G M + cpp
// samples, from the call's row and the channel's history) is read into LDS once.  Where M is even the window is stored transposed,
// sample k at (k mod M) Q + k / M, so that the G lanes of a row, M samples apart, read consecutive LDS words; where M is odd the plain
// order is already free of bank conflicts.  A design with L too large for that (G L outputs would need more LDS than a block gets) falls
// back to G = 1, 256 consecutive outputs a block with a row per lane, and one whose window does not fit even then reads its inputs
// straight from memory.  Sums run j = 0 .. cpp - 1 in fp64, the reference's order (resample.c:139-144); products may be fused.
// The blocks behind the tiles in x write the history behind the call (the last cpp - 1 inputs) into the other history buffer.
// Channels with equal designs share one copy of h.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <utility>
#include <vector>
#include "qh_design_bank.hpp"
#include "qh_design.hpp"

using namespace qh;

namespace {

constexpr int kRsBlock = 256;
constexpr int kRsLdsCap = 4096;                         // samples of a tile's window in LDS at most (64 KB complex, 32 KB real)
constexpr long long kRsMaxNcoef = 4194304;
constexpr int kRsSlots = 8;                             // calls whose phases can be in flight
constexpr int kRsCopyTile = 4096;                       // samples a block of a channel that does not run copies per grid step

struct RsParam {
    const double *h;                                    // [L][cpp]
    int L, M, cpp, run;
    int G, lg;                                          // outputs of one tap row in a tile, and its log2
    int S;                                              // rows of a tile: L, or 256 consecutive outputs where G == 1
    int Q;                                              // the transposed window's row length; 0: the window in plain order
    int lds, pad;                                       // the window fits the launch's LDS
};
static_assert(sizeof(RsParam) == 48, "the layout the kernel and the upload share");

struct RsCall { int phnum, count; };

struct RsSettings {
    int in_rate, out_rate, ncoef;
    double fc, fc_low, gain;
    int run;
};

struct RsDesign {
    int in_rate, out_rate, ncoef_in;
    double fc, fc_low, gain;
    int L, M, cpp, ncoef;
    std::vector<double> h;                              // phase-major, as on the device
    double *d_h = nullptr;
    ~RsDesign() { (void)hipFree(d_h); }
    bool is(const RsSettings &s) const
    {
        return in_rate == s.in_rate && out_rate == s.out_rate && ncoef_in == s.ncoef && fc == s.fc && fc_low == s.fc_low && gain == s.gain;
    }
};

template <bool kCplx> struct RsT;
template <> struct RsT<true> { using Io = double2; using Acc = double2; };
template <> struct RsT<false> { using Io = float; using Acc = double; };

__device__ __forceinline__ double2 rs_widen(double2 v) { return v; }
__device__ __forceinline__ double rs_widen(float v) { return (double)v; }              // resample.c:307
__device__ __forceinline__ void rs_mac(double2 &a, double t, double2 v) { a.x += t * v.x; a.y += t * v.y; }     // resample.c:142-143
__device__ __forceinline__ void rs_mac(double &a, double t, double v) { a += t * v; }                           // resample.c:316
__device__ __forceinline__ void rs_narrow(double2 *o, double2 a) { *o = a; }
__device__ __forceinline__ void rs_narrow(float *o, double a) { *o = (float)a; }       // resample.c:318
__device__ __forceinline__ double2 rs_zero(double2) { return make_double2(0.0, 0.0); }
__device__ __forceinline__ double rs_zero(double) { return 0.0; }

typedef const double __attribute__((address_space(4))) *RsTapPtr;      // read-only for the kernel's life: a uniform address loads as a scalar

// One output whose wavefront shares the tap row: `at` is the LDS word of the newest input of lane 0's output and `lane` this lane's
// distance from it; the walk (at, left) stays in scalar registers.  left: steps until the transposed window's row wraps.
template <typename Acc>
__device__ __forceinline__ Acc rs_dot_uniform(const Acc *s_x, RsTapPtr hp, int cpp, int at, int lane, int left, int Q, int wrap, int period)
{
    Acc a = rs_zero(Acc());
    for (int j = 0; j < cpp; j++) {
        rs_mac(a, hp[j], s_x[at + lane]);
        if (left == 0) { left = period - 1; at += wrap; }
        else { left--; at -= Q; }
    }
    return a;
}

// One output with a tap row of the lane's own: the same walk per lane, eight steps at a time where no wrap falls among them
template <typename Acc>
__device__ __forceinline__ Acc rs_dot_lane(const Acc *s_x, RsTapPtr hp, int cpp, int at, int left, int Q, int wrap, int period)
{
    Acc a = rs_zero(Acc());
    int j = 0;
    for (; j + 8 <= cpp; j += 8) {
        if (left >= 8) {
#pragma unroll
            for (int t = 0; t < 8; t++) rs_mac(a, hp[j + t], s_x[at - t * Q]);
            at -= 8 * Q;
            left -= 8;
        } else {
#pragma unroll
            for (int t = 0; t < 8; t++) {
                rs_mac(a, hp[j + t], s_x[at]);
                if (left == 0) { left = period - 1; at += wrap; }
                else { left--; at -= Q; }
            }
        }
    }
    for (; j < cpp; j++) {
        rs_mac(a, hp[j], s_x[at]);
        if (left == 0) { left = period - 1; at += wrap; }
        else { left--; at -= Q; }
    }
    return a;
}

// Blocks 0 .. ntiles - 1 of x: a tile of channel blockIdx.y.  The blocks behind them: the channel's history behind the call.
// History rows hold hcap samples, the newest last: hrow[hcap + g] is stream sample g < 0 of the call.
template <bool kCplx>
__global__ __launch_bounds__(kRsBlock) void resample_kernel(const typename RsT<kCplx>::Io *in, long long in_stride, typename RsT<kCplx>::Io *out,
                                                            long long out_stride, int n, const RsParam *prm, const RsCall *call,
                                                            const typename RsT<kCplx>::Acc *old_hist, typename RsT<kCplx>::Acc *new_hist, int hcap,
                                                            int ntiles)
{
    using Io = typename RsT<kCplx>::Io;
    using Acc = typename RsT<kCplx>::Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Acc *s_x = reinterpret_cast<Acc *>(s_raw);
    const int ch = blockIdx.y, tid = threadIdx.x;
    const RsParam p = prm[ch];
    const Io *irow = in + (long long)ch * in_stride;
    const Acc *hrow = old_hist + (long long)ch * hcap;
    if ((int)blockIdx.x >= ntiles) {
        // new_hist[hcap - 1 - j] <- the sample j behind the call's last one, j < cpp - 1; a channel that does not run keeps its ring
        const int j = ((int)blockIdx.x - ntiles) * kRsBlock + tid;
        if (j >= p.cpp - 1) return;
        const int slot = hcap - 1 - j;
        const long long g = (long long)n - 1 - j;
        Acc v;
        if (!p.run) v = hrow[slot];
        else if (g >= 0) v = rs_widen(irow[g]);
        else v = hrow[hcap + g];
        new_hist[(long long)ch * hcap + slot] = v;
        return;
    }
    Io *orow = out + (long long)ch * out_stride;
    if (!p.run) {                                       // resample.c:154-155, 327-328
        for (long long k = (long long)blockIdx.x * kRsCopyTile; k < n; k += (long long)ntiles * kRsCopyTile)
            for (int t = tid; t < kRsCopyTile && k + t < n; t += kRsBlock) orow[k + t] = irow[k + t];
        return;
    }
    const RsCall c = call[ch];
    const int L = p.L, M = p.M, cpp = p.cpp, G = p.G;
    const int T = p.S * G;
    const long long m0 = (long long)blockIdx.x * T;
    if (m0 >= c.count) return;
    const int valid = (int)(c.count - m0 < T ? c.count - m0 : T);
    const long long P0 = (long long)c.phnum + m0 * M;   // the upsampled position of the tile's first output
    const long long i_first = P0 / L, i_last = (P0 + (long long)(valid - 1) * M) / L;
    const long long g0 = i_first - (cpp - 1);           // the window: stream samples g0 .. i_last
    const int W = (int)(i_last - g0 + 1);
    const int Q = p.Q ? p.Q : 1;                        // sample k of the window at (k mod M) Q + k / M, or at k
    const int period = p.Q ? M : INT_MAX, wrap = p.Q ? (M - 1) * p.Q - 1 : 0;
    if (p.lds) {
        for (int k = tid; k < W; k += kRsBlock) {
            const long long g = g0 + k;
            const Acc v = g >= 0 ? rs_widen(irow[g]) : hrow[hcap + g];
            s_x[p.Q ? (k % M) * Q + k / M : k] = v;
        }
        __syncthreads();
    }
    for (int q0 = 0; q0 < T; q0 += kRsBlock) {
        const int q = q0 + tid;
        const int s = q >> p.lg, g = q & (G - 1);
        const int u = s + g * L;                        // (G == 1: g is 0 and the tile's outputs are s = 0 .. 255)
        const bool live = q < T && u < valid;
        if (G >= 64) {
            // the wavefront's 64 lanes are g = gw .. gw + 63 of row slot s
            const int sw = __builtin_amdgcn_readfirstlane(s), gw = __builtin_amdgcn_readfirstlane(g);
            if (sw >= p.S || sw + gw * L >= valid) continue;           // (uniform: the first lane's output is the wavefront's earliest)
            const long long pp = P0 + (long long)(sw + (long long)gw * L) * M;
            const int row = (int)(pp % L), k0 = (int)(pp / L - g0);
            if (!live) continue;
            RsTapPtr hp = (RsTapPtr)(p.h + (long long)row * cpp);
            const int at = p.Q ? (k0 % M) * Q + k0 / M : k0, left = p.Q ? k0 % M : INT_MAX;        // (G > 1: the window is in LDS)
            rs_narrow(&orow[m0 + u], rs_dot_uniform<Acc>(s_x, hp, cpp, at, p.Q ? g - gw : (g - gw) * M, left, Q, wrap, period));
        } else {
            if (!live) continue;
            const long long pp = P0 + (long long)u * M;
            const long long i = pp / L;
            RsTapPtr hp = (RsTapPtr)(p.h + (pp % L) * cpp);
            Acc a;
            if (p.lds) {
                const int k0 = (int)(i - g0);
                const int at = p.Q ? (k0 % M) * Q + k0 / M : k0, left = p.Q ? k0 % M : INT_MAX;
                a = rs_dot_lane<Acc>(s_x, hp, cpp, at, left, Q, wrap, period);
            } else {
                a = rs_zero(Acc());
                for (int j = 0; j < cpp; j++) {
                    const long long gi = i - j;
                    rs_mac(a, hp[j], gi >= 0 ? rs_widen(irow[gi]) : hrow[hcap + gi]);
                }
            }
            rs_narrow(&orow[m0 + u], a);
        }
    }
}

bool rs_fv(int dtype) { return dtype == QH_RESAMPLE_R32; }

const char *rs_refusal(const RsSettings &s, bool fv)
{
    if (s.in_rate <= 0 || s.out_rate <= 0) return "the rates must be positive";
    if (s.ncoef < 0) return "ncoef must not be negative";
    if (!std::isfinite(s.fc) || !std::isfinite(s.fc_low) || !std::isfinite(s.gain)) return "fc, fc_low and gain must be finite";
    int L, M;
    long long ncoef;
    resampler_sizes(s.in_rate, s.out_rate, s.ncoef, fv, &L, &M, &ncoef);
    if ((long long)s.in_rate * L > INT_MAX) return "in_rate * L must fit an int (the reference's full_rate)";
    if (ncoef > kRsMaxNcoef) return "ncoef must not exceed 4194304 coefficients after rounding up to whole rows";
    return nullptr;
}

// what a tile of G outputs a row needs of LDS, in samples; *Q: the transposed window's row length, 0 for the plain order
long long rs_need(int L, int M, int cpp, int G, int *Q)
{
    const long long T = (long long)(G > 1 ? L : kRsBlock) * G;
    const long long Wb = ((T - 1) * M + L - 1) / L + cpp;
    if (G == 1 || (M & 1)) { *Q = 0; return Wb; }
    const long long q = (Wb + M - 1) / M;
    *Q = (int)std::min<long long>(q, INT_MAX);
    return q * M;
}

}  // namespace

int qh::resample_check_settings(int in_rate, int out_rate, double fc, int ncoef, double gain, int dtype)
{
    if (dtype != QH_RESAMPLE_C64 && dtype != QH_RESAMPLE_R32) return set_error(QH_ERR_INVALID, "qh_resample_create: bad dtype");
    const char *why = rs_refusal(RsSettings{in_rate, out_rate, ncoef, fc, -1.0, gain, 1}, rs_fv(dtype));
    return why ? set_error(QH_ERR_INVALID, "qh_resample_create: %s", why) : QH_OK;
}

struct qh_resample : DesignBank<RsSettings, RsDesign, RsParam, kRsSlots> {
    int dtype = QH_RESAMPLE_C64;
    int g_first = 8;                                    // the G tried first for L >= 16: measured 2 .. 16, DESIGN.md row b23 (QH_RESAMPLE_G,
                                                        // diagnostics: a power of two, 1 .. 256, read at create)
    std::vector<int> phnum;
    RsCall *d_call = nullptr, *h_call = nullptr;        // h_call: a ring of rows in pinned host memory, a row free again when its copy has run
    void *hist[2] = { nullptr, nullptr };
    int hcap = 0;

    bool fv() const { return rs_fv(dtype); }
    size_t es_io() const { return fv() ? sizeof(float) : sizeof(double2); }
    size_t es_acc() const { return fv() ? sizeof(double) : sizeof(double2); }

    ~qh_resample()
    {
        quiesce();
        (void)hipFree(d_call); (void)hipFree(hist[0]); (void)hipFree(hist[1]);
        if (h_call) (void)hipHostFree(h_call);
    }

    const char *refusal(const RsSettings &s) const { return rs_refusal(s, fv()); }

    // The design of `s`: one a channel of the bank (or of `more`) already has, or a new one with h in device memory.  Null: the message is set.
    std::shared_ptr<RsDesign> design(const RsSettings &s, const Designs &more, const char *name)
    {
        if (auto d = cached(s, more)) return d;
        const ResamplerDesign hd = fv() ? design_resampler_fv(s.in_rate, s.out_rate) : design_resampler(s.in_rate, s.out_rate, s.fc, s.ncoef, s.gain, s.fc_low);
        auto d = std::make_shared<RsDesign>();
        d->in_rate = s.in_rate; d->out_rate = s.out_rate; d->ncoef_in = s.ncoef; d->fc = s.fc; d->fc_low = s.fc_low; d->gain = s.gain;
        d->L = hd.L; d->M = hd.M; d->cpp = hd.cpp; d->ncoef = hd.ncoef;
        d->h = resampler_phase_major(hd);
        return with_taps(d, d->h.data(), hd.ncoef, name);
    }

    void fill_param(int ch)
    {
        const RsDesign &d = *des[ch];
        int G = g_first;
        if (d.L < 16)
            for (G = 16; (long long)G * d.L < kRsBlock && G < 256;) G *= 2;
        int Q = 0;
        while (G > 1 && rs_need(d.L, d.M, d.cpp, G, &Q) > kRsLdsCap) G /= 2;
        const long long need = rs_need(d.L, d.M, d.cpp, G, &Q);
        int lg = 0;
        while ((1 << lg) < G) lg++;
        prm[ch] = RsParam{d.d_h, d.L, d.M, d.cpp, set[ch].run, G, lg, G > 1 ? d.L : kRsBlock, need <= kRsLdsCap ? Q : 0, need <= kRsLdsCap, 0};
        dirty = true;
    }

    long long lds_need(int ch) const
    {
        if (!prm[ch].lds) return 0;
        int Q;
        return rs_need(prm[ch].L, prm[ch].M, prm[ch].cpp, prm[ch].G, &Q);
    }

    // history rows of at least `want` samples: the rows move to the end of longer ones, behind everything enqueued so far
    int grow_hist(int want, const char *name)
    {
        if (want <= hcap) return QH_OK;
        want += want / 8 + 64;
        const size_t es = es_acc();
        void *nh[2] = { nullptr, nullptr };
        QH_HIP(hipStreamSynchronize(stream));
        bool ok = hipMalloc(&nh[0], (size_t)nch * want * es) == hipSuccess && hipMalloc(&nh[1], (size_t)nch * want * es) == hipSuccess;
        ok = ok && dev_zero(nh[0], (size_t)nch * want * es) == hipSuccess && dev_zero(nh[1], (size_t)nch * want * es) == hipSuccess;
        if (ok && hcap > 0)
            ok = hipMemcpy2D(static_cast<char *>(nh[cur]) + (size_t)(want - hcap) * es, (size_t)want * es, hist[cur], (size_t)hcap * es, (size_t)hcap * es,
                             (size_t)nch, hipMemcpyDeviceToDevice) == hipSuccess;
        if (!ok) {
            (void)hipFree(nh[0]); (void)hipFree(nh[1]);
            return set_error(QH_ERR_HIP, "%s: history allocation failed", name);
        }
        (void)hipFree(hist[0]); (void)hipFree(hist[1]);
        hist[0] = nh[0]; hist[1] = nh[1];
        hcap = want;
        return QH_OK;
    }

    // design_bank_set's steps: the history must hold cpp - 1 samples of the new designs; the restart reads nothing of d_prm, so the new
    // rows wait for the next call's upload
    int before_adopt(const Designs &fresh, const char *name)
    {
        int want = 0;
        for (const auto &d : fresh)
            if (d) want = std::max(want, d->cpp - 1);
        return grow_hist(want, name);
    }
    void designed(int) {}
    int before_restart() { return QH_OK; }

    // flush_resample (resample.c:113-118): the ring zeroed and phnum 0
    int restart(int ch, int)
    {
        QH_HIP(hipMemsetAsync(static_cast<char *>(hist[cur]) + (size_t)ch * hcap * es_acc(), 0, (size_t)hcap * es_acc(), stream));
        phnum[ch] = 0;
        return QH_OK;
    }

    // what channel ch makes of n samples at phase ph, and the phase behind them (resample.c:134-150 in closed form)
    long long count(int ch, int n, int ph, int *next) const
    {
        const RsDesign &d = *des[ch];
        const long long span = (long long)n * d.L;
        const long long c = span > ph ? (span - ph + d.M - 1) / d.M : 0;
        if (next) *next = (int)(ph + c * d.M - span);
        return c;
    }

    long long max_out(int n) const
    {
        long long mo = 0;
        for (int ch = 0; ch < nch; ch++) mo = std::max(mo, set[ch].run ? count(ch, n, 0, nullptr) : (long long)n);
        return mo;
    }
};

namespace {

// A setter of the band edges (a new design): the real-float form has none
template <typename F> int rs_set_edges(qh_resample *h, int ch, const char *name, F edit)
{
    if (h && ch >= -1 && ch < h->nch && h->fv())
        return set_error(QH_ERR_INVALID, "%s: the real-float form has no band edges to set (create_resampleF fixes them)", name);
    return design_bank_set(h, ch, name, 2, edit);
}

template <bool kCplx>
void rs_launch(qh_resample *h, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n, int ntiles, int nhb, size_t lds)
{
    using Io = typename RsT<kCplx>::Io;
    using Acc = typename RsT<kCplx>::Acc;
    hipLaunchKernelGGL(resample_kernel<kCplx>, dim3((unsigned)(ntiles + nhb), (unsigned)h->nch), dim3(kRsBlock), lds, h->stream, static_cast<const Io *>(d_in),
                       in_stride, static_cast<Io *>(d_out), out_stride, n, h->d_prm, h->d_call, static_cast<const Acc *>(h->hist[h->cur]),
                       static_cast<Acc *>(h->hist[h->cur ^ 1]), h->hcap, ntiles);
}

}  // namespace

extern "C" {

qh_resample *qh_resample_create(int device, int nch, int in_rate, int out_rate, double fc, int ncoef, double gain, int dtype, void *stream)
{
    if (nch <= 0 || nch > 65535) { set_error(QH_ERR_INVALID, "qh_resample_create: bad arguments"); return nullptr; }
    if (resample_check_settings(in_rate, out_rate, fc, ncoef, gain, dtype) != QH_OK) return nullptr;
    // create_resampleF has no fc, ncoef or gain (resample.c:236): the real-float form keeps the values it would be designed with
    const RsSettings s0 = rs_fv(dtype) ? RsSettings{in_rate, out_rate, 0, 0.0, -1.0, 1.0, 1} : RsSettings{in_rate, out_rate, ncoef, fc, -1.0, gain, 1};
    qh_resample *h = new qh_resample();
    h->nch = nch;
    h->dtype = dtype;
    if (const char *v = std::getenv("QH_RESAMPLE_G")) {
        const int g = std::atoi(v);
        if (g >= 1 && g <= 256 && !(g & (g - 1))) h->g_first = g;
    }
    auto fail = [&](const char *what) -> qh_resample * { set_error(QH_ERR_HIP, "qh_resample_create: %s failed", what); delete h; return nullptr; };
    if (bank_open(h, device, stream, "qh_resample_create") != QH_OK) { delete h; return nullptr; }
    h->set.assign((size_t)nch, s0);
    h->prm.assign((size_t)nch, RsParam{});
    h->phnum.assign((size_t)nch, 0);
    std::shared_ptr<RsDesign> d = h->design(s0, {}, "qh_resample_create");
    if (!d) { delete h; return nullptr; }
    h->des.assign((size_t)nch, d);
    for (int ch = 0; ch < nch; ch++) h->fill_param(ch);
    if (dev_alloc(&h->d_prm, (size_t)nch) != hipSuccess || dev_alloc(&h->d_call, (size_t)nch) != hipSuccess) return fail("hipMalloc");
    if (hipHostMalloc((void **)&h->h_call, (size_t)kRsSlots * (size_t)nch * sizeof(RsCall), hipHostMallocDefault) != hipSuccess) { h->h_call = nullptr; return fail("hipHostMalloc"); }
    if (!h->create_slots()) return fail("event creation");
    // the ring of the reference is zeroed (malloc0, resample.c:74)
    if (h->grow_hist(std::max(d->cpp - 1, 1), "qh_resample_create") != QH_OK) { delete h; return nullptr; }
    if (h->upload() != QH_OK) { delete h; return nullptr; }
    return h;
}

void qh_resample_destroy(qh_resample *h) { delete h; }

#define QH_RS_GET(name, expr)                                   \
    int name(qh_resample *h, int ch)                            \
    {                                                           \
        if (!h || ch < 0 || ch >= h->nch) return 0;             \
        std::lock_guard<std::mutex> lk(h->mtx);                 \
        return expr;                                            \
    }
QH_RS_GET(qh_resample_L, h->des[ch]->L)
QH_RS_GET(qh_resample_M, h->des[ch]->M)
QH_RS_GET(qh_resample_cpp, h->des[ch]->cpp)
#undef QH_RS_GET

int qh_resample_taps(qh_resample *h, int ch, double *out, int cap)
{
    if (!h || ch < 0 || ch >= h->nch || !out) return set_error(QH_ERR_INVALID, "qh_resample_taps: bad arguments");
    std::lock_guard<std::mutex> lk(h->mtx);
    const RsDesign &d = *h->des[ch];
    if (cap < d.ncoef) return set_error(QH_ERR_INVALID, "qh_resample_taps: room for %d coefficients, the design has %d", cap, d.ncoef);
    std::copy(d.h.begin(), d.h.end(), out);
    return d.ncoef;
}

int qh_resample_flush(qh_resample *h, int ch) { return design_bank_set(h, ch, "qh_resample_flush", 1, [](RsSettings &) { return true; }); }
int qh_resample_set_run(qh_resample *h, int ch, int run)
{
    return design_bank_set(h, ch, "qh_resample_set_run", 0, [=](RsSettings &s) { s.run = run != 0; return true; });
}
int qh_resample_set_rates(qh_resample *h, int ch, int in_rate, int out_rate)
{
    return design_bank_set(h, ch, "qh_resample_set_rates", 2, [=](RsSettings &s) { s.in_rate = in_rate; s.out_rate = out_rate; return true; });
}
int qh_resample_set_fc_low(qh_resample *h, int ch, double fc_low)
{
    return rs_set_edges(h, ch, "qh_resample_set_fc_low", [=](RsSettings &s) {
        if (fc_low == s.fc_low) return false;           // resample.c:187
        s.fc_low = fc_low;
        return true;
    });
}
int qh_resample_set_bandwidth(qh_resample *h, int ch, double fc_low, double fc_high)
{
    return rs_set_edges(h, ch, "qh_resample_set_bandwidth", [=](RsSettings &s) {
        if (fc_low == s.fc_low && fc_high == s.fc) return false;        // resample.c:197
        s.fc_low = fc_low; s.fc = fc_high;
        return true;
    });
}

long long qh_resample_out_count(qh_resample *h, int ch, int n)
{
    if (!h || ch < 0 || ch >= h->nch || n < 0) return set_error(QH_ERR_INVALID, "qh_resample_out_count: bad arguments");
    std::lock_guard<std::mutex> lk(h->mtx);
    return h->set[ch].run ? h->count(ch, n, h->phnum[ch], nullptr) : 0;
}

long long qh_resample_max_out(qh_resample *h, int n)
{
    if (!h || n < 0) return set_error(QH_ERR_INVALID, "qh_resample_max_out: bad arguments");
    std::lock_guard<std::mutex> lk(h->mtx);
    return h->max_out(n);
}

int qh_resample_process(qh_resample *h, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n, int *counts)
{
    if (!h || n < 0 || !counts || (n > 0 && (!d_in || !d_out || in_stride < n))) return set_error(QH_ERR_INVALID, "qh_resample_process: bad arguments");
    std::lock_guard<std::mutex> lk(h->mtx);
    const long long mo = h->max_out(n);
    if (mo > INT_MAX) return set_error(QH_ERR_INVALID, "qh_resample_process: %lld output samples a row do not fit the counts", mo);
    if (n > 0 && out_stride < mo) return set_error(QH_ERR_INVALID, "qh_resample_process: out_stride %lld is below qh_resample_max_out = %lld", out_stride, mo);
    const long long es = (long long)h->es_io();
    if (rows_overlap(d_in, in_stride * es, (long long)n * es, d_out, out_stride * es, mo * es, h->nch))
        return set_error(QH_ERR_INVALID, "qh_resample_process: the output rows overlap the input rows (an output is a sum over the inputs around it)");
    const int nch = h->nch;
    if (n == 0) {
        std::fill(counts, counts + nch, 0);
        return QH_OK;
    }
    QH_HIP(hipSetDevice(h->device));
    if (int rc = h->upload()) return rc;
    hipStream_t s = h->stream;
    int sl;
    if (int rc = h->take_slot(&sl)) return rc;
    RsCall *row = h->h_call + (size_t)sl * nch;
    std::vector<int> next((size_t)nch);
    long long ntiles = 1, need = 1;
    int hist_rows = 0;
    for (int ch = 0; ch < nch; ch++) {
        const RsParam &p = h->prm[ch];
        hist_rows = std::max(hist_rows, p.cpp - 1);
        if (!p.run) {
            row[ch] = RsCall{h->phnum[ch], 0};
            next[ch] = h->phnum[ch];
            ntiles = std::max(ntiles, ((long long)n + kRsCopyTile - 1) / kRsCopyTile);
            continue;
        }
        const long long c = h->count(ch, n, h->phnum[ch], &next[ch]);
        row[ch] = RsCall{h->phnum[ch], (int)c};
        const long long T = (long long)p.S * p.G;
        ntiles = std::max(ntiles, (c + T - 1) / T);
        need = std::max(need, h->lds_need(ch));
    }
    const int nhb = (hist_rows + kRsBlock - 1) / kRsBlock;
    if (ntiles + nhb > INT_MAX) return set_error(QH_ERR_INVALID, "qh_resample_process: too many tiles for one launch");
    QH_HIP(hipMemcpyAsync(h->d_call, row, (size_t)nch * sizeof(RsCall), hipMemcpyHostToDevice, s));
    if (int rc = h->slot_enqueued()) return rc;
    const size_t lds = (size_t)need * h->es_acc();
    if (h->fv()) rs_launch<false>(h, d_in, in_stride, d_out, out_stride, n, (int)ntiles, nhb, lds);
    else rs_launch<true>(h, d_in, in_stride, d_out, out_stride, n, (int)ntiles, nhb, lds);
    QH_HIP(hipGetLastError());
    h->cur ^= 1;
    for (int ch = 0; ch < nch; ch++) {
        counts[ch] = row[ch].count;
        h->phnum[ch] = next[ch];
    }
    return QH_OK;
}

int qh_resample_process_host(qh_resample *h, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n, int *counts)
{
    if (!h || n < 0 || !counts || (n > 0 && (!h_in || !h_out || in_stride < n))) return set_error(QH_ERR_INVALID, "qh_resample_process_host: bad arguments");
    const long long mo = qh_resample_max_out(h, n);
    if (mo < 0) return (int)mo;
    if (n > 0 && out_stride < mo) return set_error(QH_ERR_INVALID, "qh_resample_process_host: out_stride %lld is below qh_resample_max_out = %lld", out_stride, mo);
    QH_HIP(hipSetDevice(h->device));
    const size_t nch = (size_t)h->nch, es = h->es_io();
    void *d = nullptr, *o = nullptr;
    int rc = QH_OK;
    if (hipMalloc(&d, std::max<size_t>(nch * (size_t)n, 1) * es) != hipSuccess || hipMalloc(&o, std::max<size_t>(nch * (size_t)mo, 1) * es) != hipSuccess)
        rc = set_error(QH_ERR_HIP, "qh_resample_process_host: hipMalloc failed");
    if (rc == QH_OK && n > 0 && hipMemcpy2DAsync(d, (size_t)n * es, h_in, (size_t)in_stride * es, (size_t)n * es, nch, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        rc = set_error(QH_ERR_HIP, "qh_resample_process_host: upload failed");
    std::vector<char> run(nch);
    {
        std::lock_guard<std::mutex> lk(h->mtx);
        for (size_t ch = 0; ch < nch; ch++) run[ch] = (char)h->set[ch].run;
    }
    if (rc == QH_OK) rc = qh_resample_process(h, d, std::max(n, 1), o, std::max<long long>(mo, 1), n, counts);
    // nothing behind a row's count; a channel that does not run has its n samples copied and reports 0
    if (rc == QH_OK && n > 0) {
        hipError_t e = hipSuccess;
        for (size_t ch = 0; ch < nch && e == hipSuccess; ch++) {
            const size_t len = run[ch] ? (size_t)counts[ch] : (size_t)n;
            if (len > 0)
                e = hipMemcpyAsync(static_cast<char *>(h_out) + ch * (size_t)out_stride * es, static_cast<char *>(o) + ch * (size_t)mo * es, len * es,
                                   hipMemcpyDeviceToHost, h->stream);
        }
        if (e != hipSuccess) rc = set_error(QH_ERR_HIP, "qh_resample_process_host: download failed");
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == QH_OK) rc = set_error(QH_ERR_HIP, "qh_resample_process_host: synchronize failed");
    (void)hipFree(d); (void)hipFree(o);
    return rc;
}

int qh_resample_synchronize(qh_resample *h) { return bank_synchronize(h, "qh_resample_synchronize"); }

}  // extern "C"
