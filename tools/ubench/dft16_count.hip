// The 16-point butterflies of qh_fft.hpp alone, for an instruction count without a kernel around them:
//     python tools/isa_arith_count.py --source tools/ubench/dft16_count.hip 'dft16_count'
// (compile only; nothing here is meant to run)
#include "../../quisk_amd/csrc/qh_fft.hpp"
using namespace qh;

template <bool LEAN16, bool INV, typename C> __global__ void dft16_count(C *p)
{
    C x[16];
#pragma unroll
    for (int r = 0; r < 16; r++) x[r] = p[threadIdx.x + NT * r];
    dft16<LEAN16, INV>(x);
#pragma unroll
    for (int r = 0; r < 16; r++) p[threadIdx.x + NT * r] = x[r];
}
template __global__ void dft16_count<false, false, double2>(double2 *);
template __global__ void dft16_count<false, true, double2>(double2 *);
template __global__ void dft16_count<true, false, double2>(double2 *);
template __global__ void dft16_count<true, true, double2>(double2 *);
template __global__ void dft16_count<true, false, float2>(float2 *);      // (compiles: no fp32 tile uses it yet)
template __global__ void dft16_count<true, true, float2>(float2 *);
