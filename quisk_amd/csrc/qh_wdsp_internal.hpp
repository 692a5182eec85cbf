// qh_wdsp_internal.hpp -- what the two units of the WDSP names share: qh_wdsp_compat.cpp (the channel, its iobuffs and slews, the RXA
// setters, the wdspFexchange0 shim) and qh_wdsp_ext.cpp (the EXT and V families around the channel).
#pragma once
#include "qh_internal.hpp"

namespace qh {
namespace wdsp {

extern thread_local int g_status;                       // what qh_wdsp_status() reports: the last WDSP name's result on this thread

// Work on a stream of our own (`own`) in order with the caller's: behind what `caller` holds on entry, and `caller` behind it on return.
// Nothing is waited for on the host; caller == own needs neither.
struct StreamJoin {
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    int enter(hipStream_t caller, hipStream_t own, const char *name)
    {
        if (!ev_in && (hipEventCreateWithFlags(&ev_in, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_out, hipEventDisableTiming) != hipSuccess))
            return set_error(QH_ERR_HIP, "%s: event creation failed", name);
        if (caller != own) { (void)hipEventRecord(ev_in, caller); (void)hipStreamWaitEvent(own, ev_in, 0); }
        return QH_OK;
    }
    void leave(hipStream_t caller, hipStream_t own)
    {
        if (caller != own) { (void)hipEventRecord(ev_out, own); (void)hipStreamWaitEvent(caller, ev_out, 0); }
    }
    void release()
    {
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
        ev_in = ev_out = nullptr;
    }
};

}  // namespace wdsp
}  // namespace qh
