// qh_internal.hpp -- declarations shared by the translation units of libquiskhip.so.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/quiskhip.h"

namespace qh {

extern thread_local std::string g_last_error;

// Records the message for qh_last_error() and returns `code`.
int set_error(int code, const char *fmt, ...);

#define QH_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return qh::set_error(QH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// QH_POISON_ALLOC=1 (diagnostics): every allocation starts as NaNs / huge negative integers instead of what the allocator hands out,
// so that a buffer read before it is written shows in the results of any run, not only where the pool returns used memory
template <typename T> static inline hipError_t dev_alloc(T **p, size_t n)
{
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T));
    static const bool poison = [] { const char *v = std::getenv("QH_POISON_ALLOC"); return v && v[0] == '1'; }();
    if (e == hipSuccess && poison && n) { (void)hipMemset(*p, 0xFF, n * sizeof(T)); (void)hipDeviceSynchronize(); }
    return e;
}

// Zeros for a buffer that kernels on a NON-BLOCKING stream will use next: hipMemset runs on the null stream, which such streams do not wait
// for, and the API lets it return before the fill has run (it does not on this ROCm, but nothing promises that)
static inline hipError_t dev_zero(void *p, size_t bytes)
{
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

// Whether two matrices of rows share a byte: row c of A is [a + c sa, a + c sa + la), row c of B [b + c sb, b + c sb + lb), c < nrows (all
// in bytes).  Exact: rows of one matrix that sit in the gaps between the rows of the other are disjoint from it, whatever the extents of the
// two matrices do.  Both lists of rows ascend by start and by end, so one merge walk over them finds the first pair that meets -- O(nrows).
// A stride of 0 makes a matrix one buffer of la (lb) bytes; empty rows overlap nothing.
static inline bool rows_overlap(const void *a, long long a_stride_bytes, long long a_len_bytes, const void *b, long long b_stride_bytes,
                                long long b_len_bytes, long long nrows)
{
    if (!a || !b || a_len_bytes <= 0 || b_len_bytes <= 0 || nrows <= 0) return false;
    long long pa = (long long)reinterpret_cast<uintptr_t>(a), pb = (long long)reinterpret_cast<uintptr_t>(b);
    long long sa = a_stride_bytes, sb = b_stride_bytes;
    if (sa < 0) { pa += (nrows - 1) * sa; sa = -sa; }
    if (sb < 0) { pb += (nrows - 1) * sb; sb = -sb; }
    for (long long i = 0, j = 0; i < nrows && j < nrows;) {
        const long long a0 = pa + i * sa, b0 = pb + j * sb;
        if (a0 + a_len_bytes <= b0) i++;            // row i of A ends before row j of B, and every later row of B starts later still
        else if (b0 + b_len_bytes <= a0) j++;
        else return true;
    }
    return false;
}

// QH_OK, or QH_ERR_INVALID with the message set, for the settings qh_anb_create / qh_nob_create refuse (qh_anb.hip, qh_nob.hip): what
// lets create_anbEXT / create_nobEXT tell refused settings from a device that failed
int anb_check_settings(double samplerate, double tau, double hangtime, double advtime, double backtau, double threshold);
int nob_check_settings(double samplerate, int mode, double slewtime, double hangtime, double advtime, double backtau, double threshold);
// the same for qh_varsamp_create (qh_varsamp.hip) and create_varsampV
int varsamp_check_settings(int in_rate, int out_rate, int R, double fc, double fc_low, double gain);
// the same for qh_resample_create (qh_resample.hip) and create_resampleV / create_resampleFV
int resample_check_settings(int in_rate, int out_rate, double fc, int ncoef, double gain, int dtype);

// qh_div_process (qh_div.hip) on rows the caller has staged on the device, apart from the output rows: bit i of `alias` says that the
// caller's receiver i of every group was the very row its output goes to (xdivEXT's out == in[i]), so that it contributes the running sum
int div_process_staged(qh_div *b, const void *d_in, long long rx_stride, long long group_stride, void *d_out, long long out_stride, int n,
                       unsigned alias);

// The display bank behind a WDSP display id (XCreateAnalyzer), held until wdsp_display_release: DestroyAnalyzer waits (qh_analyzer.hip)
qh_ana *wdsp_display_hold(int disp);
void wdsp_display_release();

// gen0 set to a mode the engine refuses (4, 5) on a channel whose generator runs: the error the next process call would return, ahead
// of it -- fexchange0 asks before it takes the caller's samples, so that a refused call leaves its rings and the output buffer alone
int rxa_gen_check(qh_rxa *h);

}  // namespace qh
