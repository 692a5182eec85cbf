// qh_design_bank.hpp -- the host code the two resampler banks have in common (qh_varsamp.hip, qh_resample.hip): every channel holds a
// design -- taps in device memory that channels with equal settings share -- and a parameter row the kernels read; a call writes a row
// of a ring in host memory that the device reads, a row being free again when its call's reader has run.
#pragma once
#include <memory>
#include <utility>
#include <vector>
#include "qh_bank.hpp"

namespace qh {

// S: a channel's settings; D: a design, with is(S) and the taps d_h; P: a channel's parameter row; kSlots: the rows of the per-call ring.
template <typename S, typename D, typename P, int kSlots> struct DesignBank : Bank {
    typedef std::vector<std::shared_ptr<D>> Designs;
    std::vector<S> set;
    Designs des;
    std::vector<P> prm;
    P *d_prm = nullptr;
    hipEvent_t ev[kSlots] = {};
    bool ev_used[kSlots] = {};
    int slot = 0;

    ~DesignBank()                                       // (behind the quiesce of the bank's own destructor: no kernel reads an h any more)
    {
        (void)hipFree(d_prm);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        des.clear();
    }

    // The design a channel of the bank (or of `more`) already has for `s`, or null
    std::shared_ptr<D> cached(const S &s, const Designs &more) const
    {
        for (const Designs *list : { &des, &more })
            for (const auto &d : *list)
                if (d && d->is(s)) return d;
        return nullptr;
    }

    // d with its ncoef taps in device memory.  Null: the message is set.
    static std::shared_ptr<D> with_taps(std::shared_ptr<D> d, const double *h, int ncoef, const char *name)
    {
        if (dev_alloc(&d->d_h, (size_t)ncoef) != hipSuccess || hipMemcpy(d->d_h, h, (size_t)ncoef * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            set_error(QH_ERR_HIP, "%s: the upload of %d coefficients failed", name, ncoef);
            return nullptr;
        }
        return d;
    }

    // host settings -> device, behind everything enqueued so far
    int upload()
    {
        if (!dirty) return QH_OK;
        QH_HIP(hipStreamSynchronize(stream));
        QH_HIP(hipMemcpy(d_prm, prm.data(), (size_t)nch * sizeof(P), hipMemcpyHostToDevice));
        dirty = false;
        return QH_OK;
    }

    bool create_slots()
    {
        for (hipEvent_t &e : ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; return false; }
        return true;
    }
    // The row of this call, free to write: waits only with kSlots calls in flight
    int take_slot(int *sl)
    {
        *sl = slot;
        if (ev_used[slot]) QH_HIP(hipEventSynchronize(ev[slot]));
        return QH_OK;
    }
    // The row's reader has just been enqueued: the row is taken until it has run, the next call writes the next one
    int slot_enqueued()
    {
        QH_HIP(hipEventRecord(ev[slot], stream));
        ev_used[slot] = true;
        slot = (slot + 1) % kSlots;
        return QH_OK;
    }
};

// One setter: `edit` changes a copy of the settings of channel ch (-1: every channel) and says whether the channel is to be restarted;
// a refusal or a failed upload leaves everything as it was.  restart 0: nothing starts over; 1: flush; 2: a new design (calc_*).  The
// bank provides refusal(settings), design(settings, more, name), before_adopt(fresh, name) (what the bank must hold before it takes
// the new designs), designed(c) (channel c has just got a new design), fill_param(c), before_restart() and restart(c, mode).
template <typename B, typename F> int design_bank_set(B *h, int ch, const char *name, int restart, F edit)
{
    if (!h || ch < -1 || ch >= h->nch) return set_error(QH_ERR_INVALID, "%s: bad arguments", name);
    std::lock_guard<std::mutex> lk(h->mtx);
    const int c0 = ch < 0 ? 0 : ch, c1 = ch < 0 ? h->nch : ch + 1;
    auto next = decltype(h->set)(h->set.begin() + c0, h->set.begin() + c1);
    std::vector<char> touched((size_t)(c1 - c0), 0);
    for (int c = c0; c < c1; c++) {
        touched[c - c0] = edit(next[c - c0]) ? 1 : 0;
        if (const char *why = h->refusal(next[c - c0])) return set_error(QH_ERR_INVALID, "%s: %s", name, why);
    }
    QH_HIP(hipSetDevice(h->device));
    typename B::Designs fresh((size_t)(c1 - c0));
    if (restart == 2) {
        for (int c = c0; c < c1; c++) {
            if (!touched[c - c0]) continue;
            fresh[c - c0] = h->design(next[c - c0], fresh, name);
            if (!fresh[c - c0]) return QH_ERR_HIP;
        }
        if (int rc = h->before_adopt(fresh, name)) return rc;
        QH_HIP(hipStreamSynchronize(h->stream));       // a design nobody holds any more is freed below: no kernel may still read it
    }
    for (int c = c0; c < c1; c++) {
        h->set[c] = next[c - c0];
        if (restart == 2 && touched[c - c0]) {
            h->des[c] = fresh[c - c0];
            h->designed(c);
        }
        h->fill_param(c);
    }
    if (!restart) return QH_OK;
    if (int rc = h->before_restart()) return rc;
    for (int c = c0; c < c1; c++)
        if (touched[c - c0])
            if (int rc = h->restart(c, restart)) return rc;
    return QH_OK;
}

}  // namespace qh
