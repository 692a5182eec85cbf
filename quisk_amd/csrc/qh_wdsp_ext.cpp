// qh_wdsp_ext.cpp -- the WDSP names around the channel (include/quiskhip.h group 2): the EXT families in front of fexchange0 -- the
// blankers ANB and NOB, the diversity combiner DIV -- and the V families beside it, varsampV and resampleV / resampleFV.  Each id
// (EXT) or pointer (V) is a one-channel bank on a stream of its own with staging rows; qh_wdsp_status() (qh_wdsp_compat.cpp) reports
// what these names leave in g_status.
#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>
#include "qh_wdsp_internal.hpp"

using qh::wdsp::g_status;

namespace {

// What an id and a pointer have alike: the bank, its stream, the staging rows with their room in samples, and the caller's stream's way in
template <typename B> struct Staged {
    B *b = nullptr;
    hipStream_t stream = nullptr;
    void *d_in = nullptr, *d_out = nullptr;
    long long cap_in = 0, cap_out = 0;
    qh::wdsp::StreamJoin join;
};

template <typename B> void staged_release(Staged<B> &a, void (*destroy)(B *))
{
    if (a.b) destroy(a.b);                      // (waits for the stream)
    (void)hipFree(a.d_in); (void)hipFree(a.d_out);
    a.join.release();
    if (a.stream) (void)hipStreamDestroy(a.stream);
}

// Room for `want` elements of `es` bytes in a staging row, behind everything enqueued on `s`.  slack: the V families' calls vary in
// size, their rows grow with headroom; the EXT families' sizes are set, their rows are exactly that long.
int grow_row(hipStream_t s, void **row, long long *cap, long long want, size_t es, bool slack, const char *name)
{
    if (want <= *cap) return QH_OK;
    if (hipStreamSynchronize(s) != hipSuccess) return qh::set_error(QH_ERR_HIP, "%s: synchronize failed", name);
    (void)hipFree(*row);
    *row = nullptr; *cap = 0;
    if (slack) want += want / 8 + 64;
    if (hipMalloc(row, (size_t)want * es) != hipSuccess) { *row = nullptr; return qh::set_error(QH_ERR_HIP, "%s: staging allocation failed", name); }
    *cap = want;
    return QH_OK;
}

// ---- the EXT families: create_anbEXT ... SetEXTANBThreshold (wdsp/nob.c:307-422), the second blanker ("NB2") create_nobEXT ...
// SetEXTNOBThreshold (wdsp/nobII.c:605-734), and create_divEXT ... SetEXTDIVRotate (wdsp/div.c:104-187) ----------------------------------
// panb[id], nob.c:307-308, pnob[id], nobII.c:605-606, and pdiv[id], div.c:104-105: each id a one-channel bank on a stream of its own,
// with staging rows that let in == out
template <typename B> struct Ext : Staged<B> {
    int buffsize = 0;
};

constexpr int kMaxExtAnbs = 32;     // MAX_EXT_ANBS, nob.c:307
Ext<qh_anb> g_anb[kMaxExtAnbs];
std::recursive_mutex g_anb_mtx[kMaxExtAnbs];
constexpr int kMaxExtNobs = 32;     // MAX_EXT_NOBS, nobII.c:605
Ext<qh_nob> g_nob[kMaxExtNobs];
std::recursive_mutex g_nob_mtx[kMaxExtNobs];
constexpr int kMaxExtDivs = 32;     // (MAX_EXT_DIVS is 2, div.c:104; 32 as the other EXT families here)
constexpr int kDivRows = 8;         // MAX_NR, div.c:29
Ext<qh_div> g_div[kMaxExtDivs];
std::recursive_mutex g_div_mtx[kMaxExtDivs];

// What tells the three apart: the table, the bank's destroy, and the names the messages carry
struct AnbExt {
    typedef qh_anb Bank;
    static constexpr int count = kMaxExtAnbs;
    static Ext<qh_anb> *slots() { return g_anb; }
    static std::recursive_mutex *mutexes() { return g_anb_mtx; }
    static constexpr auto destroy = qh_anb_destroy;
    static constexpr const char *tag = "ANB", *x_host = "xanbEXT", *x_device = "qh_wdsp_xanbEXT_device";
};
struct NobExt {
    typedef qh_nob Bank;
    static constexpr int count = kMaxExtNobs;
    static Ext<qh_nob> *slots() { return g_nob; }
    static std::recursive_mutex *mutexes() { return g_nob_mtx; }
    static constexpr auto destroy = qh_nob_destroy;
    static constexpr const char *tag = "NOB", *x_host = "xnobEXT", *x_device = "qh_wdsp_xnobEXT_device";
};
struct DivExt {
    typedef qh_div Bank;
    static constexpr int count = kMaxExtDivs;
    static Ext<qh_div> *slots() { return g_div; }
    static std::recursive_mutex *mutexes() { return g_div_mtx; }
    static constexpr auto destroy = qh_div_destroy;
    static constexpr const char *tag = "DIV", *x_host = "xdivEXT", *x_device = "qh_wdsp_xdivEXT_device";
};

template <typename X> void ext_release(Ext<typename X::Bank> &a)
{
    staged_release(a, X::destroy);
    a = Ext<typename X::Bank>();
}

// The slot of a created id, locked
template <typename X> struct LockedExt {
    Ext<typename X::Bank> *a = nullptr;
    std::unique_lock<std::recursive_mutex> lk;
    explicit LockedExt(int id)
    {
        g_status = QH_OK;
        if (id < 0 || id >= X::count) { g_status = qh::set_error(QH_ERR_INVALID, "%s id %d out of range", X::tag, id); return; }
        lk = std::unique_lock<std::recursive_mutex>(X::mutexes()[id]);
        if (!X::slots()[id].b) { g_status = qh::set_error(QH_ERR_INVALID, "%s id %d has not been created", X::tag, id); return; }
        a = &X::slots()[id];
    }
};

// Staging for calls of n samples: rows_in input rows side by side (a row is cap_in samples) and one output row
template <typename B> int ext_staging(Ext<B> &a, int n, int rows_in, const char *name)
{
    if (int rc = grow_row(a.stream, &a.d_in, &a.cap_in, n, (size_t)rows_in * 16, false, name)) return rc;
    return grow_row(a.stream, &a.d_out, &a.cap_out, n, 16, false, name);
}

// create_*EXT: the id's free slot, locked, gets a stream and what `make` puts on it (the bank, the buffer size, the staging) once
// `check` has passed the settings; both return a status with the message set
template <typename X, typename C, typename M> void ext_create(int id, const char *name, C check, M make)
{
    g_status = QH_OK;
    if (id < 0 || id >= X::count) { g_status = qh::set_error(QH_ERR_INVALID, "%s id %d out of range", X::tag, id); return; }
    std::unique_lock<std::recursive_mutex> lk(X::mutexes()[id]);
    Ext<typename X::Bank> &a = X::slots()[id];
    if (a.b) { g_status = qh::set_error(QH_ERR_INVALID, "%s id %d already exists", X::tag, id); return; }
    if (int rc = check()) { g_status = rc; return; }
    if (hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking) != hipSuccess) {
        a.stream = nullptr;
        g_status = qh::set_error(QH_ERR_NO_DEVICE, "%s: no HIP device (libquiskhip has no CPU fallback)", name);
        return;
    }
    if (int rc = make(a)) { g_status = rc; ext_release<X>(a); }
}

// A blanker's `make`: the settings were good, so a bank that is not there is the device's doing (message already set)
template <typename X, typename R> int blanker_made(Ext<typename X::Bank> &a, int buffsize, R set_run, int run)
{
    if (!a.b) return QH_ERR_HIP;
    a.buffsize = buffsize;
    if (int rc = set_run(a.b, 0, run)) return rc;
    return ext_staging(a, buffsize, 1, X::x_host);
}

// x*EXT: one buffer of host samples through the bank; returns when `out` holds the result
template <typename X, typename P> void ext_x_host(int id, double *in, double *out, P process)
{
    LockedExt<X> L(id);
    if (!L.a) return;
    Ext<typename X::Bank> &a = *L.a;
    if (!in || !out) { g_status = qh::set_error(QH_ERR_INVALID, "%s: null buffer", X::x_host); return; }
    if (int rc = ext_staging(a, a.buffsize, 1, X::x_host)) { g_status = rc; return; }
    const size_t bytes = (size_t)a.buffsize * 16;
    if (hipMemcpyAsync(a.d_in, in, bytes, hipMemcpyHostToDevice, a.stream) != hipSuccess) { g_status = qh::set_error(QH_ERR_HIP, "%s: upload failed", X::x_host); return; }
    if (int rc = process(a.b, a.d_in, a.buffsize, a.d_out, a.buffsize, a.buffsize)) { g_status = rc; return; }
    if (hipMemcpyAsync(out, a.d_out, bytes, hipMemcpyDeviceToHost, a.stream) != hipSuccess || hipStreamSynchronize(a.stream) != hipSuccess)
        g_status = qh::set_error(QH_ERR_HIP, "%s: download failed", X::x_host);
}

// qh_wdsp_x*EXT_device: the same on device buffers, in order with the caller's stream
template <typename X, typename P> int ext_x_device(int id, const void *d_in, void *d_out, void *stream, P process)
{
    LockedExt<X> L(id);
    if (!L.a) return g_status;
    Ext<typename X::Bank> &a = *L.a;
    if (!d_in || !d_out) return g_status = qh::set_error(QH_ERR_INVALID, "%s: null buffer", X::x_device);
    if (int rc = ext_staging(a, a.buffsize, 1, X::x_host)) return g_status = rc;
    hipStream_t cs = (hipStream_t)stream;
    if (int rc = a.join.enter(cs, a.stream, X::x_device)) return g_status = rc;
    const size_t bytes = (size_t)a.buffsize * 16;
    int rc = QH_OK;
    if (hipMemcpyAsync(a.d_in, d_in, bytes, hipMemcpyDeviceToDevice, a.stream) != hipSuccess) rc = qh::set_error(QH_ERR_HIP, "%s: copy failed", X::x_device);
    if (!rc) rc = process(a.b, a.d_in, a.buffsize, a.d_out, a.buffsize, a.buffsize);
    if (!rc && hipMemcpyAsync(d_out, a.d_out, bytes, hipMemcpyDeviceToDevice, a.stream) != hipSuccess) rc = qh::set_error(QH_ERR_HIP, "%s: copy failed", X::x_device);
    a.join.leave(cs, a.stream);
    return g_status = rc;
}

// SetEXT*Buffsize; least: the smallest size the family takes
template <typename X> void ext_set_buffsize(int id, int size, int least, const char *name)
{
    LockedExt<X> L(id);
    if (!L.a) return;
    if (size < least) { g_status = qh::set_error(QH_ERR_INVALID, "%s: bad buffer size", name); return; }
    L.a->buffsize = size;
}

#define EXT_SETTER(X, call)                 \
    do {                                    \
        LockedExt<X> L(id);                 \
        if (L.a) g_status = (call);         \
    } while (0)

// DIV: the caller's receivers are pointers of their own, the bank's are rows a stride apart: the rows a call reads are gathered into
// d_in [8][cap_in] first, and the receivers whose pointer is `out` go to the bank as a mask (qh::div_process_staged), so out == in[k]
// needs no copy to undo.
// What a call of nsamples on pointers in[0 .. nr-1] / out reads and where out lies over it (host or device addresses alike): the first
// row read and their count, the receivers whose pointer is out, and whether nothing is to be done (a copy of in[output] onto itself)
struct DivCall {
    int first = 0, count = 0;
    unsigned alias = 0;
    bool nothing = false;
};

int div_call(Ext<qh_div> &a, int nsamples, const void *const *in, const void *out, const char *name, DivCall *c)
{
    int run = 0, nr = 0, output = 0;
    if (int rc = qh_div_get(a.b, 0, &run, &nr, &output, nullptr, nullptr)) return rc;
    if (nsamples < 0 || !in || !out) return qh::set_error(QH_ERR_INVALID, "%s: bad arguments", name);
    if (run && output > nr) return qh::set_error(QH_ERR_INVALID, "%s: output %d is above nr %d (the reference reads a receiver nobody handed it)", name, output, nr);
    const bool mix = run && output == nr;
    c->first = !run || mix ? 0 : output;
    c->count = mix ? nr : 1;
    const long long o = (long long)reinterpret_cast<uintptr_t>(out), len = (long long)nsamples * 16;
    for (int i = c->first; i < c->first + c->count; i++) {
        if (!in[i]) return qh::set_error(QH_ERR_INVALID, "%s: in[%d] is null", name, i);
        const long long p = (long long)reinterpret_cast<uintptr_t>(in[i]);
        if (p == o) c->alias |= 1u << i;
        else if (p < o + len && o < p + len) return qh::set_error(QH_ERR_INVALID, "%s: out overlaps in[%d] without being it", name, i);
    }
    c->nothing = nsamples == 0 || (!mix && c->alias);
    return QH_OK;
}

// Receiver i's row of the gathered input
double *div_row(Ext<qh_div> &a, int i) { return static_cast<double *>(a.d_in) + (size_t)i * (size_t)a.cap_in * 2; }

}  // namespace

extern "C" {

void create_anbEXT(int id, int run, int buffsize, double samplerate, double tau, double hangtime, double advtime, double backtau, double threshold)
{
    ext_create<AnbExt>(id, "create_anbEXT",
        [&] { return buffsize <= 0 ? qh::set_error(QH_ERR_INVALID, "create_anbEXT: bad buffer size") : qh::anb_check_settings(samplerate, tau, hangtime, advtime, backtau, threshold); },
        [&](Ext<qh_anb> &a) {
            a.b = qh_anb_create(0, 1, samplerate, tau, hangtime, advtime, backtau, threshold, a.stream);
            return blanker_made<AnbExt>(a, buffsize, qh_anb_set_run, run);
        });
}

void destroy_anbEXT(int id) { LockedExt<AnbExt> L(id); if (L.a) ext_release<AnbExt>(*L.a); }
void flush_anbEXT(int id) { EXT_SETTER(AnbExt, qh_anb_flush(L.a->b, 0)); }
void xanbEXT(int id, double *in, double *out) { ext_x_host<AnbExt>(id, in, out, qh_anb_process); }
int qh_wdsp_xanbEXT_device(int id, const void *d_in, void *d_out, void *stream) { return ext_x_device<AnbExt>(id, d_in, d_out, stream, qh_anb_process); }

void SetEXTANBRun(int id, int run) { EXT_SETTER(AnbExt, qh_anb_set_run(L.a->b, 0, run)); }
void SetEXTANBBuffsize(int id, int size) { ext_set_buffsize<AnbExt>(id, size, 1, "SetEXTANBBuffsize"); }
void SetEXTANBSamplerate(int id, int rate) { EXT_SETTER(AnbExt, qh_anb_set_samplerate(L.a->b, 0, (double)rate)); }
void SetEXTANBTau(int id, double tau) { EXT_SETTER(AnbExt, qh_anb_set_tau(L.a->b, 0, tau)); }
void SetEXTANBHangtime(int id, double time) { EXT_SETTER(AnbExt, qh_anb_set_hangtime(L.a->b, 0, time)); }
void SetEXTANBAdvtime(int id, double time) { EXT_SETTER(AnbExt, qh_anb_set_advtime(L.a->b, 0, time)); }
void SetEXTANBBacktau(int id, double tau) { EXT_SETTER(AnbExt, qh_anb_set_backtau(L.a->b, 0, tau)); }
void SetEXTANBThreshold(int id, double thresh) { EXT_SETTER(AnbExt, qh_anb_set_threshold(L.a->b, 0, thresh)); }

void create_nobEXT(int id, int run, int mode, int buffsize, double samplerate, double slewtime, double hangtime, double advtime, double backtau,
                   double threshold)
{
    ext_create<NobExt>(id, "create_nobEXT",
        [&] { return buffsize <= 0 ? qh::set_error(QH_ERR_INVALID, "create_nobEXT: bad buffer size") : qh::nob_check_settings(samplerate, mode, slewtime, hangtime, advtime, backtau, threshold); },
        [&](Ext<qh_nob> &a) {
            a.b = qh_nob_create(0, 1, samplerate, mode, slewtime, hangtime, advtime, backtau, threshold, a.stream);
            return blanker_made<NobExt>(a, buffsize, qh_nob_set_run, run);
        });
}

void destroy_nobEXT(int id) { LockedExt<NobExt> L(id); if (L.a) ext_release<NobExt>(*L.a); }
void flush_nobEXT(int id) { EXT_SETTER(NobExt, qh_nob_flush(L.a->b, 0)); }
void xnobEXT(int id, double *in, double *out) { ext_x_host<NobExt>(id, in, out, qh_nob_process); }
int qh_wdsp_xnobEXT_device(int id, const void *d_in, void *d_out, void *stream) { return ext_x_device<NobExt>(id, d_in, d_out, stream, qh_nob_process); }

void SetEXTNOBRun(int id, int run) { EXT_SETTER(NobExt, qh_nob_set_run(L.a->b, 0, run)); }
void SetEXTNOBMode(int id, int mode) { EXT_SETTER(NobExt, qh_nob_set_mode(L.a->b, 0, mode)); }
void SetEXTNOBBuffsize(int id, int size) { ext_set_buffsize<NobExt>(id, size, 1, "SetEXTNOBBuffsize"); }
void SetEXTNOBSamplerate(int id, int rate) { EXT_SETTER(NobExt, qh_nob_set_samplerate(L.a->b, 0, (double)rate)); }
void SetEXTNOBTau(int id, double tau) { EXT_SETTER(NobExt, qh_nob_set_tau(L.a->b, 0, tau)); }
void SetEXTNOBHangtime(int id, double time) { EXT_SETTER(NobExt, qh_nob_set_hangtime(L.a->b, 0, time)); }
void SetEXTNOBAdvtime(int id, double time) { EXT_SETTER(NobExt, qh_nob_set_advtime(L.a->b, 0, time)); }
void SetEXTNOBBacktau(int id, double tau) { EXT_SETTER(NobExt, qh_nob_set_backtau(L.a->b, 0, tau)); }
void SetEXTNOBThreshold(int id, double thresh) { EXT_SETTER(NobExt, qh_nob_set_threshold(L.a->b, 0, thresh)); }

void create_divEXT(int id, int run, int nr, int size)
{
    ext_create<DivExt>(id, "create_divEXT",
        [&] { return size < 0 || nr < 1 || nr > kDivRows ? qh::set_error(QH_ERR_INVALID, "create_divEXT: nr must lie in 1..8 and the size must not be negative") : (int)QH_OK; },
        [&](Ext<qh_div> &a) {
            a.b = qh_div_create(0, 1, run, nr, a.stream);
            if (!a.b) return (int)QH_ERR_HIP;           // the settings were good: the device (message already set)
            a.buffsize = size;
            return ext_staging(a, size, kDivRows, "create_divEXT");
        });
}

void destroy_divEXT(int id) { LockedExt<DivExt> L(id); if (L.a) ext_release<DivExt>(*L.a); }
void flush_divEXT(int id) { LockedExt<DivExt> L(id); }                    // flush_div is empty, div.c:62-65

void xdivEXT(int id, int nsamples, double **in, double *out)
{
    LockedExt<DivExt> L(id);
    if (!L.a) return;
    Ext<qh_div> &a = *L.a;
    DivCall c;
    if (int rc = div_call(a, nsamples, (const void *const *)in, out, DivExt::x_host, &c)) { g_status = rc; return; }
    if (c.nothing) return;
    if (int rc = ext_staging(a, nsamples, kDivRows, DivExt::x_host)) { g_status = rc; return; }
    const size_t bytes = (size_t)nsamples * 16;
    for (int i = c.first; i < c.first + c.count; i++)
        if (!((c.alias >> i) & 1u) &&                                       // (the samples of a receiver that is `out` are never read)
            hipMemcpyAsync(div_row(a, i), in[i], bytes, hipMemcpyHostToDevice, a.stream) != hipSuccess) {
            (void)hipStreamSynchronize(a.stream);
            g_status = qh::set_error(QH_ERR_HIP, "%s: upload failed", DivExt::x_host);
            return;
        }
    int rc = qh::div_process_staged(a.b, a.d_in, a.cap_in, (long long)kDivRows * a.cap_in, a.d_out, a.cap_out, nsamples, c.alias);
    if (!rc && hipMemcpyAsync(out, a.d_out, bytes, hipMemcpyDeviceToHost, a.stream) != hipSuccess) rc = qh::set_error(QH_ERR_HIP, "%s: download failed", DivExt::x_host);
    if (hipStreamSynchronize(a.stream) != hipSuccess && !rc) rc = qh::set_error(QH_ERR_HIP, "%s: download failed", DivExt::x_host);
    g_status = rc;
}

int qh_wdsp_xdivEXT_device(int id, int nsamples, const void *const *d_in, void *d_out, void *stream)
{
    LockedExt<DivExt> L(id);
    if (!L.a) return g_status;
    Ext<qh_div> &a = *L.a;
    DivCall c;
    if (int rc = div_call(a, nsamples, d_in, d_out, DivExt::x_device, &c)) return g_status = rc;
    if (c.nothing) return QH_OK;
    if (int rc = ext_staging(a, nsamples, kDivRows, DivExt::x_device)) return g_status = rc;
    hipStream_t cs = (hipStream_t)stream;
    if (int rc = a.join.enter(cs, a.stream, DivExt::x_device)) return g_status = rc;
    const size_t bytes = (size_t)nsamples * 16;
    int rc = QH_OK;
    for (int i = c.first; i < c.first + c.count && !rc; i++)
        if (!((c.alias >> i) & 1u) && hipMemcpyAsync(div_row(a, i), d_in[i], bytes, hipMemcpyDeviceToDevice, a.stream) != hipSuccess)
            rc = qh::set_error(QH_ERR_HIP, "%s: copy failed", DivExt::x_device);
    if (!rc) rc = qh::div_process_staged(a.b, a.d_in, a.cap_in, (long long)kDivRows * a.cap_in, d_out, nsamples, nsamples, c.alias);
    a.join.leave(cs, a.stream);
    return g_status = rc;
}

void SetEXTDIVRun(int id, int run) { EXT_SETTER(DivExt, qh_div_set_run(L.a->b, 0, run)); }
void SetEXTDIVBuffsize(int id, int size) { ext_set_buffsize<DivExt>(id, size, 0, "SetEXTDIVBuffsize"); }
void SetEXTDIVNr(int id, int nr) { EXT_SETTER(DivExt, qh_div_set_nr(L.a->b, 0, nr)); }
void SetEXTDIVOutput(int id, int output) { EXT_SETTER(DivExt, qh_div_set_output(L.a->b, 0, output)); }
void SetEXTDIVRotate(int id, int nr, double *Irotate, double *Qrotate) { EXT_SETTER(DivExt, qh_div_set_rotate(L.a->b, 0, nr, Irotate, Qrotate)); }

}  // extern "C"

// ---- the V families: create_varsampV, xvarsampV, destroy_varsampV (wdsp/varsamp.c:228-250) behind fexchange0, and create_resampleV,
// xresampleV, destroy_resampleV with the FV names (wdsp/resample.c:206-228, 332-354) beside it ------------------------------------------------
// Every pointer a one-channel bank on a stream of its own, with an input staging row that lets input == output and an output staging
// row for the host form.  The reference hands out its VARSAMP / RESAMPLE; here the pointer is looked up in its family's table, so one
// that the family's create did not return is refused instead of followed.
namespace {
template <typename B> struct VRec : Staged<B> {
    std::mutex mtx;                             // one call at a time on a pointer
};

// R: a family's record, a VRec with the bank's `destroy`
template <typename R> void v_release(R *a)
{
    staged_release(*a, R::destroy);
    delete a;
}

template <typename R> struct PtrTable {
    std::mutex mtx;
    std::vector<R *> list;

    // A new record on a stream of its own that `make` has put the bank on (it returns a status, the message set), entered; or null
    template <typename M> R *create(const char *name, M make)
    {
        g_status = QH_OK;
        R *a = new R();
        if (hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess) {
            a->stream = nullptr;
            g_status = qh::set_error(QH_ERR_NO_DEVICE, "%s: no HIP device (libquiskhip has no CPU fallback)", name);
        } else if (int rc = make(*a)) g_status = rc;
        else {
            std::lock_guard<std::mutex> lk(mtx);
            list.push_back(a);
            return a;
        }
        v_release(a);
        return nullptr;
    }
    // The record `ptr` is, if `maker` returned it and `ok` takes it
    template <typename Ok> R *find(void *ptr, const char *name, const char *maker, Ok ok)
    {
        g_status = QH_OK;
        std::lock_guard<std::mutex> lk(mtx);
        for (R *a : list)
            if (a == ptr && ok(*a)) return a;
        g_status = qh::set_error(QH_ERR_INVALID, "%s: not a pointer %s returned", name, maker);
        return nullptr;
    }
    // Out of the table -- no new call finds it -- then behind the call that may still hold it, then released
    void destroy(R *a)
    {
        {
            std::lock_guard<std::mutex> lk(mtx);
            list.erase(std::find(list.begin(), list.end(), a));
        }
        { std::lock_guard<std::mutex> lk(a->mtx); }
        v_release(a);
    }
};

struct VarsampV : VRec<qh_varsamp> {
    static constexpr auto destroy = qh_varsamp_destroy;
    int *d_count = nullptr;                     // the count in device memory
    ~VarsampV() { (void)hipFree(d_count); }     // (behind the bank's destroy, which waits for the stream)
};
PtrTable<VarsampV> g_vsv;

VarsampV *vsv_find(void *ptr, const char *name) { return g_vsv.find(ptr, name, "create_varsampV", [](const VarsampV &) { return true; }); }

// One table holds both kinds of resampler, so a V pointer handed to an FV name is refused as well
struct ResampleV : VRec<qh_resample> {
    static constexpr auto destroy = qh_resample_destroy;
    bool fv = false;
    size_t es() const { return fv ? sizeof(float) : 2 * sizeof(double); }
};
PtrTable<ResampleV> g_rsv;

// fv < 0: either kind
ResampleV *rsv_find(void *ptr, int fv, const char *name)
{
    return g_rsv.find(ptr, name, fv > 0 ? "create_resampleFV" : "create_resampleV", [=](const ResampleV &a) { return fv < 0 || a.fv == (fv != 0); });
}

void *rsv_create(int in_rate, int out_rate, bool fv, const char *name)
{
    g_status = QH_OK;
    const int dtype = fv ? QH_RESAMPLE_R32 : QH_RESAMPLE_C64;
    if (int rc = qh::resample_check_settings(in_rate, out_rate, 0.0, 0, 1.0, dtype)) { g_status = rc; return nullptr; }
    return g_rsv.create(name, [&](ResampleV &a) {
        a.fv = fv;
        a.b = qh_resample_create(0, 1, in_rate, out_rate, 0.0, 0, 1.0, dtype, a.stream);           // resample.c:211, 337
        return a.b ? QH_OK : QH_ERR_HIP;        // the settings were good: the device (message already set)
    });
}

void rsv_destroy(void *ptr, bool fv, const char *name)
{
    if (ResampleV *a = rsv_find(ptr, fv, name)) g_rsv.destroy(a);
}

// resample.c:130-152 with out == in: output m is written behind the input it is made at only while m <= p / L, which holds for every m
// where L <= M; where L > M the reference overwrites inputs it has yet to read
bool rsv_in_place_ok(ResampleV &a) { return qh_resample_L(a.b, 0) <= qh_resample_M(a.b, 0); }

void rsv_x(const void *input, void *output, int numsamps, int *outsamps, void *ptr, bool fv, const char *name)
{
    if (outsamps) *outsamps = 0;
    ResampleV *a = rsv_find(ptr, fv, name);
    if (!a) return;
    std::lock_guard<std::mutex> lk(a->mtx);
    if (!outsamps || numsamps < 0 || (numsamps > 0 && (!input || !output))) { g_status = qh::set_error(QH_ERR_INVALID, "%s: bad arguments", name); return; }
    if (numsamps > 0 && input == output && !rsv_in_place_ok(*a)) {
        g_status = qh::set_error(QH_ERR_INVALID, "%s: input == output needs L <= M (the reference overwrites samples it has yet to read)", name);
        return;
    }
    const long long mo = qh_resample_max_out(a->b, numsamps);
    if (mo < 0) { g_status = (int)mo; return; }
    const size_t es = a->es();
    if (int rc = grow_row(a->stream, &a->d_in, &a->cap_in, numsamps, es, true, name)) { g_status = rc; return; }
    if (int rc = grow_row(a->stream, &a->d_out, &a->cap_out, mo, es, true, name)) { g_status = rc; return; }
    if (numsamps > 0 && hipMemcpyAsync(a->d_in, input, (size_t)numsamps * es, hipMemcpyHostToDevice, a->stream) != hipSuccess) {
        g_status = qh::set_error(QH_ERR_HIP, "%s: upload failed", name);
        return;
    }
    int count = 0;
    if (int rc = qh_resample_process(a->b, a->d_in, std::max(numsamps, 1), a->d_out, std::max<long long>(mo, 1), numsamps, &count)) { g_status = rc; return; }
    if ((count > 0 && hipMemcpyAsync(output, a->d_out, (size_t)count * es, hipMemcpyDeviceToHost, a->stream) != hipSuccess) ||
        hipStreamSynchronize(a->stream) != hipSuccess) {
        g_status = qh::set_error(QH_ERR_HIP, "%s: download failed", name);
        return;
    }
    *outsamps = count;
}

int rsv_x_device(void *ptr, const void *d_in, void *d_out, int numsamps, int *outsamps, void *stream, bool fv, const char *name)
{
    if (outsamps) *outsamps = 0;
    ResampleV *a = rsv_find(ptr, fv, name);
    if (!a) return g_status;
    std::lock_guard<std::mutex> lk(a->mtx);
    if (numsamps < 0 || !outsamps || (numsamps > 0 && (!d_in || !d_out))) return g_status = qh::set_error(QH_ERR_INVALID, "%s: bad arguments", name);
    if (numsamps > 0 && d_in == d_out && !rsv_in_place_ok(*a))
        return g_status = qh::set_error(QH_ERR_INVALID, "%s: d_in == d_out needs L <= M (the reference overwrites samples it has yet to read)", name);
    const long long mo = qh_resample_max_out(a->b, numsamps);
    if (mo < 0) return g_status = (int)mo;
    if (int rc = grow_row(a->stream, &a->d_in, &a->cap_in, numsamps, a->es(), true, name)) return g_status = rc;
    hipStream_t cs = (hipStream_t)stream;
    if (int rc = a->join.enter(cs, a->stream, name)) return g_status = rc;
    int rc = QH_OK;
    if (numsamps > 0 && hipMemcpyAsync(a->d_in, d_in, (size_t)numsamps * a->es(), hipMemcpyDeviceToDevice, a->stream) != hipSuccess)
        rc = qh::set_error(QH_ERR_HIP, "%s: copy failed", name);
    if (!rc) rc = qh_resample_process(a->b, a->d_in, std::max(numsamps, 1), d_out, std::max<long long>(mo, 1), numsamps, outsamps);
    a->join.leave(cs, a->stream);
    return g_status = rc;
}
}  // namespace

extern "C" {

void *create_varsampV(int in_rate, int out_rate, int R)
{
    g_status = QH_OK;
    if (int rc = qh::varsamp_check_settings(in_rate, out_rate, R, 0.0, -1.0, 1.0)) { g_status = rc; return nullptr; }
    return g_vsv.create("create_varsampV", [&](VarsampV &a) {
        a.b = qh_varsamp_create(0, 1, in_rate, out_rate, R, 0.0, -1.0, 1.0, 1.0, 1, a.stream);     // varsamp.c:233
        if (!a.b) return (int)QH_ERR_HIP;       // the settings were good: the device (message already set)
        if (hipMalloc((void **)&a.d_count, sizeof(int)) != hipSuccess) {
            a.d_count = nullptr;
            return qh::set_error(QH_ERR_HIP, "create_varsampV: allocation failed");
        }
        return (int)QH_OK;
    });
}

void destroy_varsampV(void *ptr)
{
    if (VarsampV *a = vsv_find(ptr, "destroy_varsampV")) g_vsv.destroy(a);
}

long long qh_wdsp_varsampV_max_out(void *ptr, int numsamps, double var)
{
    VarsampV *a = vsv_find(ptr, "qh_wdsp_varsampV_max_out");
    if (!a) return g_status;
    const long long mo = qh_varsamp_max_out(a->b, numsamps, &var);
    if (mo < 0) g_status = (int)mo;
    return mo;
}

void xvarsampV(double *input, double *output, int numsamps, double var, int *outsamps, void *ptr)
{
    if (outsamps) *outsamps = 0;
    VarsampV *a = vsv_find(ptr, "xvarsampV");
    if (!a) return;
    std::lock_guard<std::mutex> lk(a->mtx);
    if (!outsamps || numsamps < 0 || (numsamps > 0 && (!input || !output))) { g_status = qh::set_error(QH_ERR_INVALID, "xvarsampV: bad arguments"); return; }
    const long long mo = qh_varsamp_max_out(a->b, numsamps, &var);
    if (mo < 0) { g_status = (int)mo; return; }
    if (int rc = grow_row(a->stream, &a->d_in, &a->cap_in, numsamps, 16, true, "xvarsampV")) { g_status = rc; return; }
    if (int rc = grow_row(a->stream, &a->d_out, &a->cap_out, mo, 16, true, "xvarsampV")) { g_status = rc; return; }
    if (numsamps > 0 && hipMemcpyAsync(a->d_in, input, (size_t)numsamps * 16, hipMemcpyHostToDevice, a->stream) != hipSuccess) {
        g_status = qh::set_error(QH_ERR_HIP, "xvarsampV: upload failed");
        return;
    }
    if (int rc = qh_varsamp_process(a->b, a->d_in, std::max(numsamps, 1), a->d_out, std::max<long long>(mo, 1), numsamps, &var, a->d_count)) { g_status = rc; return; }
    int count = 0;
    if (hipMemcpyAsync(&count, a->d_count, sizeof(int), hipMemcpyDeviceToHost, a->stream) != hipSuccess || hipStreamSynchronize(a->stream) != hipSuccess) {
        g_status = qh::set_error(QH_ERR_HIP, "xvarsampV: download failed");
        return;
    }
    if (count > 0 && (hipMemcpyAsync(output, a->d_out, (size_t)count * 16, hipMemcpyDeviceToHost, a->stream) != hipSuccess ||
                      hipStreamSynchronize(a->stream) != hipSuccess)) {
        g_status = qh::set_error(QH_ERR_HIP, "xvarsampV: download failed");
        return;
    }
    *outsamps = count;
}

int qh_wdsp_xvarsampV_device(void *ptr, const void *d_in, void *d_out, int numsamps, double var, int *d_count, void *stream)
{
    VarsampV *a = vsv_find(ptr, "qh_wdsp_xvarsampV_device");
    if (!a) return g_status;
    std::lock_guard<std::mutex> lk(a->mtx);
    if (numsamps < 0 || !d_count || (numsamps > 0 && (!d_in || !d_out))) return g_status = qh::set_error(QH_ERR_INVALID, "qh_wdsp_xvarsampV_device: bad arguments");
    const long long mo = qh_varsamp_max_out(a->b, numsamps, &var);
    if (mo < 0) return g_status = (int)mo;
    if (int rc = grow_row(a->stream, &a->d_in, &a->cap_in, numsamps, 16, true, "qh_wdsp_xvarsampV_device")) return g_status = rc;
    hipStream_t cs = (hipStream_t)stream;
    if (int rc = a->join.enter(cs, a->stream, "qh_wdsp_xvarsampV_device")) return g_status = rc;
    int rc = QH_OK;
    if (numsamps > 0 && hipMemcpyAsync(a->d_in, d_in, (size_t)numsamps * 16, hipMemcpyDeviceToDevice, a->stream) != hipSuccess)
        rc = qh::set_error(QH_ERR_HIP, "qh_wdsp_xvarsampV_device: copy failed");
    if (!rc) rc = qh_varsamp_process(a->b, a->d_in, std::max(numsamps, 1), d_out, std::max<long long>(mo, 1), numsamps, &var, d_count);
    a->join.leave(cs, a->stream);
    return g_status = rc;
}

void *create_resampleV(int in_rate, int out_rate) { return rsv_create(in_rate, out_rate, false, "create_resampleV"); }
void *create_resampleFV(int in_rate, int out_rate) { return rsv_create(in_rate, out_rate, true, "create_resampleFV"); }
void destroy_resampleV(void *ptr) { rsv_destroy(ptr, false, "destroy_resampleV"); }
void destroy_resampleFV(void *ptr) { rsv_destroy(ptr, true, "destroy_resampleFV"); }
void xresampleV(double *input, double *output, int numsamps, int *outsamps, void *ptr) { rsv_x(input, output, numsamps, outsamps, ptr, false, "xresampleV"); }
void xresampleFV(float *input, float *output, int numsamps, int *outsamps, void *ptr) { rsv_x(input, output, numsamps, outsamps, ptr, true, "xresampleFV"); }

long long qh_wdsp_resampleV_max_out(void *ptr, int numsamps)
{
    ResampleV *a = rsv_find(ptr, -1, "qh_wdsp_resampleV_max_out");
    if (!a) return g_status;
    const long long mo = qh_resample_max_out(a->b, numsamps);
    if (mo < 0) g_status = (int)mo;
    return mo;
}

int qh_wdsp_xresampleV_device(void *ptr, const void *d_in, void *d_out, int numsamps, int *outsamps, void *stream)
{
    return rsv_x_device(ptr, d_in, d_out, numsamps, outsamps, stream, false, "qh_wdsp_xresampleV_device");
}
int qh_wdsp_xresampleFV_device(void *ptr, const void *d_in, void *d_out, int numsamps, int *outsamps, void *stream)
{
    return rsv_x_device(ptr, d_in, d_out, numsamps, outsamps, stream, true, "qh_wdsp_xresampleFV_device");
}

}  // extern "C"
