// qh_taps.hpp -- the two data taps of xrxa: xsender (wdsp/sender.c:66-86, RXA.c:570) and xsiphon (wdsp/siphon.c:96-130, RXA.c:590).
// Neither changes the signal.  The sender narrows the listed channels' rows behind nbp0 to float pairs for a display; the siphon keeps
// the newest kSipSize samples of the audio behind xwcpagc in a ring whose write index lives beside it on the device, so that a
// replayed launch sequence (which bakes in its kernels' arguments) moves on through the ring like the plain path.
#pragma once
#include <hip/hip_runtime.h>
#include "qh_kernels.hpp"

namespace qh {

static constexpr int kSipSize = 4096;       // create_rxa's sipsize (RXA.c:392-401); a power of two (siphon.c:63)

// xsender mode 0 (sender.c:75-80): (dINREAL) of both parts, the chain's (I, Q) order kept; one 16-byte load and one 8-byte store a sample
static __global__ __launch_bounds__(NT) void sender_tap_kernel(const double2 *buf, long long stride, int n, const int *chan_list, float2 *rows,
                                                               long long rows_stride)
{
    const int ch = chan_list[blockIdx.y];
    const double2 *p = buf + (long long)ch * stride;
    float2 *q = rows + (long long)ch * rows_stride;
    for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
        const double2 v = p[i];
        q[i] = make_float2((float)v.x, (float)v.y);
    }
}

// xsiphon mode 0 over a call of n = nblk * insize samples.  insize < kSipSize: every block is written at idx, which moves on by insize
// (siphon.c:109-121) -- sample i of the call lands at (idx + i) mod kSipSize, and only the newest kSipSize of them are still there at the
// end.  insize >= kSipSize: every block leaves its last kSipSize samples at the ring's start and idx alone (siphon.c:105-106); the last
// block's stay.  gain: xwcpagc mode 0's multiply where the chain applies it behind this point (the output matrix), 1.0 elsewhere.
static __global__ __launch_bounds__(NT) void siphon_tap_kernel(const double2 *buf, long long stride, int n, int insize, const int *chan_list,
                                                               const double *gain, double2 *ring, const int *idx)
{
    const int ch = chan_list[blockIdx.y];
    const double g = gain[ch];
    const double2 *p = buf + (long long)ch * stride;
    double2 *r = ring + (long long)ch * kSipSize;
    const int m = n < kSipSize ? n : kSipSize, first = n - m;
    const int at = insize >= kSipSize ? 0 : (int)(((long long)idx[ch] + first) & (kSipSize - 1));
    for (int j = blockIdx.x * NT + threadIdx.x; j < m; j += gridDim.x * NT) {
        const double2 v = p[first + j];
        r[(at + j) & (kSipSize - 1)] = make_double2(g * v.x, g * v.y);
    }
}

// idx += n mod kSipSize for the listed channels, behind the launch above (insize < kSipSize only)
static __global__ void siphon_advance_kernel(int n, const int *chan_list, int count, int *idx)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int ch = chan_list[k];
    idx[ch] = (int)(((long long)idx[ch] + n) & (kSipSize - 1));
}

}  // namespace qh
