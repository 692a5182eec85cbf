// qh_design.hpp -- host-side filter design and table generation for the HIP receive chain.
// These run at parameter-change time only (the reference does the same work in
// calc_resample / fir_bandpass / calc_fircore on the setter's thread).
#pragma once
#include <complex>
#include <utility>
#include <vector>

namespace qh {

using cd = std::complex<double>;

// WDSP windowed-sinc bandpass, wdsp/fir.c:187-254.
//   rtype 0: N real taps returned as complex with zero imaginary part
//   rtype 1: N complex taps  c*cos(w n) - j*c*sin(w n)
// wintype 0 = 4-term Blackman-Harris, 1 = 7-term (fir.c:220-236).
std::vector<cd> fir_bandpass(int N, double f_low, double f_high, double samplerate, int wintype, int rtype, double scale);

// WDSP resampler prototype, wdsp/resample.c:35-72: taps in natural (time) order, real.
// Returns L, M and the tap count; `gain` as in create_resample.
struct ResamplerDesign { int L, M, ncoef, cpp; std::vector<double> h; };
ResamplerDesign design_resampler(int in_rate, int out_rate, double fc, int ncoef, double gain, double fc_low = -1.0);
// fc_low >= 0 is the lower band edge in Hz (resample.c:60-63, setFCLow_resample / setBandwidth_resample); below 0 selects -fc, and the
// taps are then the ones the five-argument call always gave.
// create_resampleF's design (resample.c:250-273): fc = 0.45 min_rate, ncoef = (int)(60 / fc_norm) rounded up to a whole row per phase,
// gain 1.  resampler_sizes: L, M and the rounded ncoef of either design in 64 bits, for the caller's refusals (rates must be positive).
// resampler_phase_major: h[L][cpp] as calc_resample stores it (resample.c:69-72).
ResamplerDesign design_resampler_fv(int in_rate, int out_rate);
void resampler_sizes(int in_rate, int out_rate, int ncoef_in, bool fv, int *L, int *M, long long *ncoef);
std::vector<double> resampler_phase_major(const ResamplerDesign &d);

// WDSP variable-ratio resampler prototype, calc_varsamp (wdsp/varsamp.c:29-68): nom_ratio = out_rate / in_rate, rsize = (int)(140 *
// norm_rate / min_rate) taps per output sample, and the R-times oversampled low-pass h of ncoef = rsize * R + 1 real coefficients
// (fir_bandpass at samplerate R, 7-term window, scale R * gain).  fc = 0 selects 0.95 * 0.45 * min_rate, fc_low < 0 selects -fc.
// Rates and R must be positive (the caller checks, and caps ncoef).
struct VarsampDesign { double nom_ratio; int rsize, ncoef; std::vector<double> h; };
void varsamp_sizes(int in_rate, int out_rate, int R, int *rsize, long long *ncoef);
VarsampDesign design_varsamp(int in_rate, int out_rate, int R, double fc, double fc_low, double gain);

// WDSP FM de-emphasis curve by frequency sampling, wdsp/fcurve.c:29-145 + fir.c:129-185 (even nc).
std::vector<cd> fc_impulse(int nc, double f0, double f1, double g0, double g1, int curve, double samplerate,
                           double scale, int ctfmode, int wintype);

// WDSP's piecewise-linear-in-dB frequency-sampling design, wdsp/eq.c:39-158 through fir_fsamp (fir.c:127-185), even N (odd N throws).
// F[1..nfreqs] in Hz and G[1..nfreqs] in dB are the design points (any order), G[0] the preamp in dB; F[0] is not read.
std::vector<cd> eq_impulse(int N, int nfreqs, const double *F, const double *G, double samplerate, double scale, int ctfmode, int wintype);
// calc_fmd's pllpole (wdsp/fmd.c:39) and the FM squelch's noise filter made from it (calc_fmsq, wdsp/fmsq.c:36-44; RXA.c:222-223)
double fm_pllpole(double zeta, double omegaN);
std::vector<cd> fmsq_impulse(int nc, double samplerate, double scale);

// Unnormalised forward DFT (power of two), double data with long double twiddles.
void host_fft(std::vector<cd> &x, int sign);

// Frequency-domain mask for qh::osfir_kernel: FFT_NFFT(h zero padded) / NFFT.
// WDSP notch database entry and the notched band-pass design, wdsp/nbp.c:64-179
struct Notch { double fcenter, fwidth; int active; };
std::vector<std::pair<double, double>> make_nbp(const std::vector<Notch> &notches, double minwidth, int autoincr, double flow,
                                                double fhigh, bool *havnotch);
std::vector<cd> fir_mbandpass(int N, const std::vector<std::pair<double, double>> &bands, double rate, double scale, int wintype);
std::vector<cd> mp_imp(const std::vector<cd> &fir, int pfactor, int polarity);     // wdsp/fir.c:319-368
std::vector<cd> make_mask(const std::vector<cd> &h, int nfft);

// calc_speak, design 1 with create_rxa's four stages (wdsp/iir.c:180-214): the one biquad the stages share and the input gain.
// f below 200 Hz is taken as 200 Hz, as the reference stores it back.
struct SpeakDesign { double a0, a1, a2, b1, b2, fgain; };
SpeakDesign design_speak(double f, double bw, double gain, double rate);

// The sweep of WDSP's signal generator (wdsp/gen.c:49-55, 246-261) by the reference's own chain: dphs starts at TWOPI f1 / rate,
// `phs += dphs; dphs += d2phs` once a sample with phs wrapped into [0, 2 pi), and the sample whose sum exceeds dphsmax = TWOPI f2 / rate
// resets dphs.  P: the samples from one reset to the next (the same every period: a reset restarts from the same expression), 0 when
// the chain never gets there (d2phs <= 0 and the first sum does not exceed).  The instants hang on the sums' rounding -- at the defaults
// exact arithmetic gives a tie that the chain decides one sample earlier -- so P is counted, not solved for.  ck: (phs, dphs) of the chain
// every ck_step samples of a period, phs from 0 at the reset; full: phs when the period ends.  Where the closed-form estimate of P
// exceeds max_walk additions the chain is not walked: P is the closed form's count (floor((dphsmax - dphs) / d2phs) + 1), ck stays
// empty, full is the exact quadratic's, and `walked` is false.
struct SweepWalk { long long P = 0; double dphs0 = 0.0, d2phs = 0.0, full = 0.0; bool walked = true; std::vector<std::pair<double, double>> ck; };
SweepWalk sweep_walk(double rate, double f1, double f2, double sweeprate, long long max_walk, int ck_step);

// Concatenated per-pass twiddle tables for qh::FftRR<N> (see the Plan table in qh_fft.hpp).
std::vector<cd> fft_twiddle_table(int n);

}  // namespace qh
