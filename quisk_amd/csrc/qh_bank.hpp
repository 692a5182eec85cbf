// qh_bank.hpp -- the host code the channel banks around the receiver have in common: a handle is `nch` streams on one device and one HIP
// stream, with settings that another thread may change between calls.  Who takes what:
//   Bank, bank_open, bank_synchronize               qh_anb.hip, qh_nob.hip, qh_div.hip, qh_varsamp.hip, qh_resample.hip
//   DetBank (the detector's scratch), bank_grow     qh_anb.hip, qh_nob.hip, and det_enqueue of qh_blank_det.hpp
//   bank_set                                        qh_anb.hip, qh_nob.hip, qh_div.hip (the resamplers' setter is in qh_design_bank.hpp)
//   bank_check_rows, bank_process_host              qh_anb.hip, qh_nob.hip
// qh_nb.hip, whose handle is a struct of its own, takes bank_open, bank_process_host and bank_synchronize.
#pragma once
#include <mutex>
#include <vector>
#include "qh_internal.hpp"

namespace qh {

// What every bank holds besides its own settings, tables and history.
struct Bank {
    int device = 0, nch = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::mutex mtx;                                     // setters may come from another thread than process (cs_update)
    bool dirty = true;                                  // host settings newer than the device's
    int cur = 0;                                        // which of a bank's two history buffers is the current one
    void quiesce()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
    ~Bank()                                             // (a bank's own destructor has freed its buffers behind a quiesce of its own)
    {
        quiesce();
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

// A blanker bank: the handle and the per-call scratch of the detector (qh_blank_det.hpp), grown with n: [nch][nt] tile values,
// [nch][nw] words of bits.  Freed behind a quiesce, before ~Bank destroys the stream.
struct DetBank : Bank {
    int cap = 0;
    long long nt = 0, nw = 0;
    double *d_ends = nullptr;
    unsigned long long *d_trb = nullptr;
    void free_scratch()
    {
        (void)hipFree(d_ends); (void)hipFree(d_trb);
        d_ends = nullptr; d_trb = nullptr; cap = 0;
    }
    ~DetBank()
    {
        quiesce();
        free_scratch();
    }
};

// The device made current and the stream of a new handle: the caller's, or a non-blocking one of the handle's own.
template <typename H> int bank_open(H *h, int device, void *stream, const char *what)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return set_error(QH_ERR_NO_DEVICE, "no HIP device %d (libquiskhip has no CPU fallback)", device);
    h->device = device;
    if (hipSetDevice(device) != hipSuccess) return set_error(QH_ERR_HIP, "%s: %s failed", what, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    if (!s) {
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return set_error(QH_ERR_HIP, "%s: %s failed", what, "stream creation");
        h->own_stream = true;
    }
    h->stream = s;
    return QH_OK;
}

// The detector's scratch for calls of up to n samples, in tiles of `tile` samples; behind everything enqueued so far when it grows.
static inline int bank_grow(DetBank *h, int n, int tile, const char *what)
{
    if (n <= h->cap) return QH_OK;
    QH_HIP(hipStreamSynchronize(h->stream));
    h->free_scratch();
    h->nw = ((long long)n + 63) / 64 + 1;
    h->nt = ((long long)n + tile - 1) / tile + 1;
    if (dev_alloc(&h->d_ends, (size_t)h->nch * (size_t)h->nt) != hipSuccess || dev_alloc(&h->d_trb, (size_t)h->nch * (size_t)h->nw) != hipSuccess) {
        h->free_scratch();
        return set_error(QH_ERR_HIP, "%s: scratch allocation failed", what);
    }
    h->cap = n;
    return QH_OK;
}

// One setter: `edit` changes a copy of the settings of channel ch (-1: every channel); a refusal leaves everything as it was.  The bank
// provides set[], refusal(settings), derive(ch) (everything from the settings, for a setter that restarts the channel), apply_light(ch)
// (the fields a setter that does not restart may change) and restart(c0, count).
template <typename B, typename F> int bank_set(B *h, int ch, const char *name, bool restart, F edit)
{
    if (!h || ch < -1 || ch >= h->nch) return set_error(QH_ERR_INVALID, "%s: bad arguments", name);
    std::lock_guard<std::mutex> lk(h->mtx);
    const int c0 = ch < 0 ? 0 : ch, c1 = ch < 0 ? h->nch : ch + 1;
    auto next = decltype(h->set)(h->set.begin() + c0, h->set.begin() + c1);
    for (auto &s : next) {
        edit(s);
        if (const char *why = B::refusal(s)) return set_error(QH_ERR_INVALID, "%s: %s", name, why);
    }
    QH_HIP(hipSetDevice(h->device));
    for (int c = c0; c < c1; c++) {
        h->set[c] = next[c - c0];
        if (restart) h->derive(c);
        else { h->apply_light(c); h->dirty = true; }
    }
    return restart ? h->restart(c0, c1 - c0) : QH_OK;
}

template <typename H> bool bank_args_ok(const H *h, const void *in, long long in_stride, const void *out, long long out_stride, int n)
{
    return h && n >= 0 && (n == 0 || (in && out && in_stride >= n && out_stride >= n));
}

// The arguments of a process call on device rows of fp64 complex samples; `why`: what the bank reads that forbids overlapping rows.
template <typename H>
int bank_check_rows(const char *name, const H *h, const void *d_in, long long in_stride, const void *d_out, long long out_stride, int n, const char *why)
{
    if (!bank_args_ok(h, d_in, in_stride, d_out, out_stride, n)) return set_error(QH_ERR_INVALID, "%s: bad arguments", name);
    if (rows_overlap(d_in, in_stride * 16, (long long)n * 16, d_out, out_stride * 16, (long long)n * 16, h->nch))
        return set_error(QH_ERR_INVALID, "%s: the output rows overlap the input rows (%s)", name, why);
    return QH_OK;
}

// Host rows through `process`: device copies of the call's size, made and freed here; returns when the output is in h_out.
template <typename H, typename P>
int bank_process_host(H *h, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n, P process, const char *name)
{
    if (!bank_args_ok(h, h_in, in_stride, h_out, out_stride, n)) return set_error(QH_ERR_INVALID, "%s: bad arguments", name);
    if (n == 0) return QH_OK;
    QH_HIP(hipSetDevice(h->device));
    double2 *d = nullptr, *o = nullptr;
    QH_HIP(hipMalloc((void **)&d, (size_t)h->nch * (size_t)n * sizeof(double2)));
    if (hipMalloc((void **)&o, (size_t)h->nch * (size_t)n * sizeof(double2)) != hipSuccess) { (void)hipFree(d); return set_error(QH_ERR_HIP, "hipMalloc failed"); }
    int rc = QH_OK;
    if (hipMemcpy2DAsync(d, (size_t)n * 16, h_in, (size_t)in_stride * 16, (size_t)n * 16, (size_t)h->nch, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        rc = set_error(QH_ERR_HIP, "upload failed");
    if (rc == QH_OK) rc = process(h, d, n, o, n, n);
    if (rc == QH_OK && hipMemcpy2DAsync(h_out, (size_t)out_stride * 16, o, (size_t)n * 16, (size_t)n * 16, (size_t)h->nch, hipMemcpyDeviceToHost,
                                         h->stream) != hipSuccess)
        rc = set_error(QH_ERR_HIP, "download failed");
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == QH_OK) rc = set_error(QH_ERR_HIP, "synchronize failed");
    (void)hipFree(d); (void)hipFree(o);
    return rc;
}

template <typename H> int bank_synchronize(H *h, const char *name)
{
    if (!h) return set_error(QH_ERR_INVALID, "%s: null handle", name);
    QH_HIP(hipSetDevice(h->device));
    QH_HIP(hipStreamSynchronize(h->stream));
    return QH_OK;
}

}  // namespace qh
