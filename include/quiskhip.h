/* quiskhip.h -- C ABI of libquiskhip.so: MI355X (gfx950) receive DSP for Quisk / WDSP.
 *
 * Plain C, plain pointers and sizes; no C++ or torch types.  Three groups of entry points:
 *
 *  1. qh_rxa_*    batched many-channel RXA engine (device-resident buffers).  The reference has
 *                 no batched form: it runs one DSP thread per channel (wdsp/channel.c:31-35) and
 *                 caps channels at 32 (wdsp/comm.h:117).  This is what bench.py measures.
 *  2. WDSP names  OpenChannel / fexchange0 / SetRXA* ... with the reference's exact signatures,
 *                 so that quisk_wdsp.py's ctypes.CDLL("./wdsp/libwdsp.so") (quisk_wdsp.py:27-41)
 *                 and quisk_wdsp.c's function pointer (quisk_wdsp.c:22,57) bind unchanged.
 *  3. qh_fir_*    batched FIR / decimator primitives equivalent to filter.c (filter.h:39-55).
 *
 * All functions returning int return 0 on success and a negative qh_status on failure;
 * qh_last_error() gives the message.  Nothing here falls back to the CPU: without a usable
 * HIP device every compute entry point fails with QH_ERR_NO_DEVICE.
 */
#ifndef QUISKHIP_H
#define QUISKHIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    QH_OK = 0,
    QH_ERR_NO_DEVICE = -1,
    QH_ERR_INVALID = -2,
    QH_ERR_UNSUPPORTED = -3,
    QH_ERR_HIP = -4
} qh_status;

/* ------------------------------------------------------------------ library */
int qh_version(void);                       /* 100 * major + minor */
const char *qh_last_error(void);            /* thread-local message of the last failure */
int qh_device_count(void);                  /* number of visible HIP devices (0 without a GPU) */

/* RXA demodulator modes, numerically identical to wdsp/RXA.h:31-45 */
enum { QH_LSB = 0, QH_USB, QH_DSB, QH_CWL, QH_CWU, QH_FM, QH_AM, QH_DIGU, QH_SPEC, QH_DIGL, QH_SAM, QH_DRM };

/* ------------------------------------------------------------------ 1. batched RXA engine */
typedef struct qh_rxa qh_rxa;

/* Creates `nch` independent receiver channels, each configured exactly like
 * OpenChannel(ch, *, dsp_size, in_rate, dsp_rate, out_rate, type 0, ...) followed by create_rxa()
 * (wdsp/channel.c:75-103, wdsp/RXA.c:31-490): shift run=1 at 0 Hz, nbp0 -4150..-150 Hz nc 2048,
 * AGC mode 3, panel gain 4.  `stream` is a hipStream_t (NULL = the engine creates its own).
 * in_rate / dsp_rate = 1, 2, 4, 8 or 16 runs the fused overlap-save front stage; any other whole ratio up or down (3, 5,
 * 6 ...; 1/2, 1/4 ...: what pre_main_build's integer divisions size consistently, wdsp/channel.c:39-42) runs xshift and the
 * polyphase resampler of wdsp/resample.c:35-157 as two passes.  out_rate: an integer multiple or fraction of dsp_rate. */
qh_rxa *qh_rxa_create(int device, int nch, int dsp_size, int in_rate, int dsp_rate, int out_rate, void *stream);
void qh_rxa_destroy(qh_rxa *e);

int qh_rxa_nch(const qh_rxa *e);
int qh_rxa_dsp_insize(const qh_rxa *e);     /* complex input samples per DSP block  (wdsp/channel.c:39-42) */
int qh_rxa_dsp_outsize(const qh_rxa *e);    /* complex output samples per DSP block (wdsp/channel.c:44-47) */
void *qh_rxa_stream(const qh_rxa *e);                            /* the hipStream_t the engine launches on */
/* Launch-sequence replay for block-at-a-time callers (the WDSP drop-in switches it on).  While the arguments of
 * qh_rxa_process and every parameter stand still, the launches of a call are captured into hipGraphs -- one per
 * state of the engine's ping-pong history buffers -- and replayed; a setter, a flush or different arguments drop
 * them.  Results are those of the plain path.  Off by default: a caller that passes large batches gains nothing. */
int qh_rxa_set_graph_replay(qh_rxa *e, int on);
long long qh_rxa_graph_launches(const qh_rxa *e);                /* calls served by a replayed graph so far */
/* Tile of the fircore (nbp0 / bp1 / bpsnba / FM audio) stages for nc <= 2048: 4096 points (0 = default), or 8192 points
 * shared by two lane groups: three times the useful outputs per pair of transforms and 22 % fewer instructions per sample, yet
 * slower on MI355X because its barriers hold eight wavefronts; kept selectable for that comparison.
 * nc = 4096 always runs 8192-point tiles, nc = 8192 ... 65536 two ... sixteen 4096-tap partitions on them.  Results agree to rounding; a change rebuilds the filter masks on the next call.
 * qh_rxa_band_tile: the size in use. */
int qh_rxa_set_band_tile(qh_rxa *e, int nfft);
int qh_rxa_band_tile(const qh_rxa *e);
/* Form of xsnba.  0 (default): one kernel per call with both of the blanker's resamplers inside its block loop where that kernel can
 * run (dsp_rate up to 48000 and dsp_size up to 1024); elsewhere, and everywhere with 1: three passes -- dsp_rate -> 12 kHz for the
 * whole call, the frames on 12 kHz rows, 12 kHz -> dsp_rate.  The results agree in every bit and the state is one
 * layout, so the form may change between calls; kept selectable for the comparison.  qh_rxa_snba_form: the value set. */
int qh_rxa_set_snba_form(qh_rxa *e, int form);
int qh_rxa_snba_form(const qh_rxa *e);

/* Per-channel setters; `ch` indexes the batch, or -1 for every channel.  Same meaning as the WDSP
 * export of the same name (cited in section 2).  They take effect at the next qh_rxa_process call,
 * i.e. on a DSP-block boundary, which is when the reference applies them (csDSP, wdsp/main.c:41). */
int qh_rxa_SetRXAMode(qh_rxa *e, int ch, int mode);
int qh_rxa_RXASetPassband(qh_rxa *e, int ch, double f_low, double f_high);
int qh_rxa_RXASetNC(qh_rxa *e, int ch, int nc);     /* a power of two in [dsp_size, 65536]; above 4096: partitions of 4096 taps (tests/test_gpu_long_nc.py) */
int qh_rxa_SetRXAShiftRun(qh_rxa *e, int ch, int run);
int qh_rxa_SetRXAShiftFreq(qh_rxa *e, int ch, double fshift);
int qh_rxa_RXANBPSetRun(qh_rxa *e, int ch, int run);
int qh_rxa_RXANBPSetFreqs(qh_rxa *e, int ch, double flow, double fhigh);
int qh_rxa_SetRXABandpassRun(qh_rxa *e, int ch, int run);
int qh_rxa_SetRXABandpassFreqs(qh_rxa *e, int ch, double f_low, double f_high);
int qh_rxa_SetRXAAGCMode(qh_rxa *e, int ch, int mode);
int qh_rxa_SetRXAAGCFixed(qh_rxa *e, int ch, double fixed_agc_db);
int qh_rxa_SetRXAAGCAttack(qh_rxa *e, int ch, int attack_ms);
int qh_rxa_SetRXAAGCDecay(qh_rxa *e, int ch, int decay_ms);
int qh_rxa_SetRXAAGCHang(qh_rxa *e, int ch, int hang_ms);
int qh_rxa_SetRXAAGCTop(qh_rxa *e, int ch, double max_agc_db);
int qh_rxa_SetRXAAGCSlope(qh_rxa *e, int ch, int slope);
int qh_rxa_SetRXAAGCHangThreshold(qh_rxa *e, int ch, int hangthreshold);
int qh_rxa_SetRXAPanelGain1(qh_rxa *e, int ch, double gain);
int qh_rxa_SetRXAPanelGain2(qh_rxa *e, int ch, double gainI, double gainQ);
int qh_rxa_SetRXAPanelSelect(qh_rxa *e, int ch, int select);
int qh_rxa_SetRXAPanelCopy(qh_rxa *e, int ch, int copy);
int qh_rxa_SetRXAPanelPan(qh_rxa *e, int ch, double pan);       /* wdsp/patchpanel.c:158-176: writes gain2I / gain2Q, as SetRXAPanelGain2 does (the last writer wins); a pan that is not finite: QH_ERR_INVALID */
int qh_rxa_SetRXAPanelBinaural(qh_rxa *e, int ch, int bin);     /* wdsp/patchpanel.c:186-192: copy = 1 - bin, the field SetRXAPanelCopy writes */
/* The AGC's display-side knobs (wdsp/wcpAGC.c:440-557): host arithmetic on the values loadWcpAGC derives from the channel's settings
 * (wcpAGC.c:115-146: out_target, min_volts, hang_level; create_rxa's out_targ 1.0 and n_tau 4, RXA.c:335-358).  A setter takes effect at
 * the next process call; a getter (one channel, not -1) reads the host's settings and waits for nothing on the device.
 *   SetRXAAGCThresh   max_gain = out_target / (var_gain 10^((thresh + noise_offset) / 20)), noise_offset = 10 log10((nbp0.fhigh -
 *                     nbp0.flow) size / rate) with nbp0's edges at the moment of the call (a later RXANBPSetFreqs does not move max_gain)
 *                     and the caller's display FFT size and rate
 *   GetRXAAGCThresh   20 log10(min_volts) - noise_offset
 *   SetRXAAGCHangLevel     max_input > min_volts: hang_thresh = 1 + 0.125 log10(max(1e-8, (10^(level / 20) - min_volts) / (max_input -
 *                     min_volts))), else 1 -- the field SetRXAAGCHangThreshold writes as percent / 100
 *   GetRXAAGCHangLevel     20 log10(hang_level / 0.637);  GetRXAAGCHangThreshold  (int)(100 hang_thresh);  GetRXAAGCTop  20 log10(max_gain)
 * Refused with QH_ERR_INVALID, nothing changed (the reference checks none of this): an argument that is not finite; size or rate not
 * above 0; an nbp0 band that is not wider than 0 (the reference would take the log of it); a thresh so far out that max_gain would not be
 * a finite number above 0; a max_input that is not above 0. */
int qh_rxa_SetRXAAGCThresh(qh_rxa *e, int ch, double thresh, double size, double rate);     /* wdsp/wcpAGC.c:499-511 */
int qh_rxa_GetRXAAGCThresh(qh_rxa *e, int ch, double *thresh, double size, double rate);    /* wdsp/wcpAGC.c:487-497 */
int qh_rxa_SetRXAAGCHangLevel(qh_rxa *e, int ch, double hangLevel);                         /* wdsp/wcpAGC.c:449-466 */
int qh_rxa_GetRXAAGCHangLevel(qh_rxa *e, int ch, double *hangLevel);                        /* wdsp/wcpAGC.c:440-447 */
int qh_rxa_GetRXAAGCHangThreshold(qh_rxa *e, int ch, int *hangthreshold);                   /* wdsp/wcpAGC.c:468-475 */
int qh_rxa_GetRXAAGCTop(qh_rxa *e, int ch, double *max_agc);                                /* wdsp/wcpAGC.c:513-520 */
int qh_rxa_SetRXAAGCMaxInputLevel(qh_rxa *e, int ch, double level);                         /* wdsp/wcpAGC.c:550-557 */
int qh_rxa_SetRXAAMDSBMode(qh_rxa *e, int ch, int sbmode);
int qh_rxa_SetRXAAMDRun(qh_rxa *e, int ch, int run);             /* wdsp/amd.c:264-277; run = 1 on a channel in FM mode (both detectors in a row in the reference) is refused at the next process call */
int qh_rxa_SetRXAFMLimRun(qh_rxa *e, int ch, int run);           /* wdsp/fmd.c:336-347: the FM detector's limiter */
int qh_rxa_SetRXAFMLimGain(qh_rxa *e, int ch, double gaindB);    /* wdsp/fmd.c:349-362 */
/* xemnr, WDSP's spectral noise reduction "NR2" (wdsp/emnr.c; setters :1096-1143): overlap-add STFT 4096 / 1024, noise estimate by
 * minimum statistics (npe 0), speech presence (npe 1) or LambdaDl (npe 2), gain methods 0 Gaussian-amplitude, 1 log-MMSE, 2 gamma tables, 3 trained
 * zeta tables, post-filter aepf; position 0 (before bp1 and the AGC) or 1.  The tables are the data WDSP loads at create time from
 * its files `calculus` (GG, GGS: 241 x 241 doubles each) and `zetaHat.bin` (60 x 60 doubles, 60 x 60 int validity flags, ranges in
 * dB): hand them over once per engine before switching EMNR on.  dsp_size up to 1024. */
int qh_rxa_SetEMNRTables(qh_rxa *e, const double *GG, const double *GGS, const double *zeta_hat, const int *zeta_valid, double gamma_min,
                         double gamma_max, double xi_min, double xi_max);
int qh_rxa_SetRXAEMNRRun(qh_rxa *e, int ch, int run);
int qh_rxa_SetRXAEMNRgainMethod(qh_rxa *e, int ch, int method);
int qh_rxa_SetRXAEMNRnpeMethod(qh_rxa *e, int ch, int method);
int qh_rxa_SetRXAEMNRaeRun(qh_rxa *e, int ch, int run);
int qh_rxa_SetRXAEMNRPosition(qh_rxa *e, int ch, int position);
int qh_rxa_SetRXAEMNRaeZetaThresh(qh_rxa *e, int ch, double v);
int qh_rxa_SetRXAEMNRaePsi(qh_rxa *e, int ch, double v);
int qh_rxa_SetRXAEMNRtrainZetaThresh(qh_rxa *e, int ch, double v);
int qh_rxa_SetRXAEMNRtrainT2(qh_rxa *e, int ch, double v);
/* xamsqcap / xamsq, the AM squelch (wdsp/amsq.c:119-192; create_amsq arguments RXA.c:158-172) */
int qh_rxa_SetRXAAMSQRun(qh_rxa *e, int ch, int run);
/* SNBA, wdsp/snb.c:579-593 (run; also switches bpsnba and bp1 as RXA.c:800-917) and :660-694 (pass band of its output resampler;
 * RXASetPassband calls it).  dsp_rate 12000 x 2^k, k = 0 .. 5 (12000 ... 384000: calc_snba's whole ratios to its 12 kHz internal rate),
 * dsp_size a multiple of dsp_rate / 12000 and at most 4096; anything else is refused when the blanker is first needed, or by the
 * rate / size setters below while a channel runs it. */
int qh_rxa_SetRXASNBARun(qh_rxa *e, int ch, int run);
int qh_rxa_SetRXASNBAOutputBandwidth(qh_rxa *e, int ch, double flow, double fhigh);
/* the blanker's tuning, wdsp/snb.c:604-658 (defaults: create_rxa's 64, 2, 8.0, 20.0, 10, 2, 2, 0.5; SetRXASNBAovrlp is not provided) */
int qh_rxa_SetRXASNBAasize(qh_rxa *e, int ch, int size);
int qh_rxa_SetRXASNBAnpasses(qh_rxa *e, int ch, int npasses);
int qh_rxa_SetRXASNBAk1(qh_rxa *e, int ch, double k1);
int qh_rxa_SetRXASNBAk2(qh_rxa *e, int ch, double k2);
int qh_rxa_SetRXASNBAbridge(qh_rxa *e, int ch, int bridge);
int qh_rxa_SetRXASNBApresamps(qh_rxa *e, int ch, int presamps);
int qh_rxa_SetRXASNBApostsamps(qh_rxa *e, int ch, int postsamps);
int qh_rxa_SetRXASNBApmultmin(qh_rxa *e, int ch, double pmultmin);
int qh_rxa_SetRXASNBAovrlp(qh_rxa *e, int ch, int ovrlp);          /* snb.c:595; ch = -1: the frame advance is the engine's */
/* xcbl, xspeak, xmpeak between the agc meter and the panel (wdsp/RXA.c:591-593), all off at create (RXA.c:403-445): the carrier block
 * (wdsp/cblock.c:120-126), the CW audio peak filter (wdsp/iir.c:322-360: design 1, four stages; the design setters zero its state) and
 * the two-tone peak filter (wdsp/iir.c:490-548: the sum of its enabled peaks; each peak's design setters zero that peak's state).
 * npeaks outside [0, 2] and fil outside [0, 2) are refused with QH_ERR_INVALID (the reference indexes past its two-peak arrays). */
int qh_rxa_SetRXACBLRun(qh_rxa *e, int ch, int run);                            /* wdsp/cblock.c:120-126 */
int qh_rxa_SetRXASPCWRun(qh_rxa *e, int ch, int run);                           /* wdsp/iir.c:322-329 */
int qh_rxa_SetRXASPCWFreq(qh_rxa *e, int ch, double freq);                      /* wdsp/iir.c:331-339 */
int qh_rxa_SetRXASPCWBandwidth(qh_rxa *e, int ch, double bw);                   /* wdsp/iir.c:341-349 */
int qh_rxa_SetRXASPCWGain(qh_rxa *e, int ch, double gain);                      /* wdsp/iir.c:351-359 */
int qh_rxa_SetRXAmpeakRun(qh_rxa *e, int ch, int run);                          /* wdsp/iir.c:490-497 */
int qh_rxa_SetRXAmpeakNpeaks(qh_rxa *e, int ch, int npeaks);                    /* wdsp/iir.c:499-506 */
int qh_rxa_SetRXAmpeakFilEnable(qh_rxa *e, int ch, int fil, int enable);        /* wdsp/iir.c:508-515 */
int qh_rxa_SetRXAmpeakFilFreq(qh_rxa *e, int ch, int fil, double freq);         /* wdsp/iir.c:517-526 */
int qh_rxa_SetRXAmpeakFilBw(qh_rxa *e, int ch, int fil, double bw);             /* wdsp/iir.c:528-537 */
int qh_rxa_SetRXAmpeakFilGain(qh_rxa *e, int ch, int fil, double gain);         /* wdsp/iir.c:539-548 */
/* xssql, the syllabic squelch between xmpeak and the panel (wdsp/RXA.c:594), off at create (RXA.c:447-461); a channel that turns it on
 * starts muted.  No setter flushes; qh_rxa_flush zeroes its blocker, crossing ring and low-pass only (ssql.c:208-220).  The threshold
 * setter keeps threshold / 2.  A tau below 0 or not finite, or a threshold that is not finite, is refused with QH_ERR_INVALID. */
int qh_rxa_SetRXASSQLRun(qh_rxa *e, int ch, int run);                           /* wdsp/ssql.c:330-336 */
int qh_rxa_SetRXASSQLThreshold(qh_rxa *e, int ch, double threshold);            /* wdsp/ssql.c:338-346 */
int qh_rxa_SetRXASSQLTauMute(qh_rxa *e, int ch, double tau_mute);               /* wdsp/ssql.c:348-358 */
int qh_rxa_SetRXASSQLTauUnMute(qh_rxa *e, int ch, double tau_unmute);           /* wdsp/ssql.c:360-370 */
/* xfmsq, the FM noise squelch right behind xfmd (wdsp/RXA.c:575), off at create with thresholds 0.750 / 0.562 (RXA.c:214-234; not 0.9
 * apart until the threshold setter runs); a channel that turns it on starts muted and stays so for the 0.1 s ready delay.  While it is
 * off nothing of it runs and its noise filter, averages and state stay as they were.  qh_rxa_flush does flush_fmsq (fmsq.c:122-130).
 * A threshold that is not finite is refused with QH_ERR_INVALID.  nc: a power of two in [dsp_size, 4096]; a larger one is accepted by the
 * setter (RXASetNC forwards here) and refused with QH_ERR_UNSUPPORTED at the next process call while the channel runs the stage.  Refused
 * there too: FMSQ on a channel whose FM detector is off, a dsp rate at or below twice the FM loop's pole (about 15.8 kHz), and FMSQ
 * channels of one engine with different nc or mp (they share one noise filter). */
int qh_rxa_SetRXAFMSQRun(qh_rxa *e, int ch, int run);                           /* wdsp/fmsq.c:235-241 */
int qh_rxa_SetRXAFMSQThreshold(qh_rxa *e, int ch, double threshold);            /* wdsp/fmsq.c:243-250: tail = threshold, unmute = 0.9 threshold */
int qh_rxa_SetRXAFMSQNC(qh_rxa *e, int ch, int nc);                             /* wdsp/fmsq.c:252-267 */
int qh_rxa_SetRXAFMSQMP(qh_rxa *e, int ch, int mp);                             /* wdsp/fmsq.c:269-279 */
/* xeqp, the receive equalizer between xsnba and xanf (wdsp/RXA.c:579), off at create with ten frequencies 32 ... 16000 Hz at 0 dB, nc
 * max(2048, dsp_size), mp 0, ctfmode 0, wintype 0 (RXA.c:257-275).  The filter is designed on the host (eq_impulse, eq.c:39-158) at the
 * next process call and runs as a fircore stage of its own with one design per channel.  While a channel's equalizer is off nothing of it
 * runs and its delay line stays as it was; SetRXAEQNC with a new nc zeroes the line, every other setter keeps it; qh_rxa_flush zeroes it
 * (flush_eqp).  F and G hold nfreqs + 1 values: G[0] is the preamp in dB, F[0] is not read.  Refused by the setter with QH_ERR_INVALID,
 * changing nothing: an nc that is not a power of two in [dsp_size, 65536], nfreqs < 1, a value of F or G that is not finite, a null
 * pointer.  Refused with QH_ERR_UNSUPPORTED at the next process call while the channel runs the stage, nothing run: an nc above 4096,
 * and a profile in which two frequencies coincide after the clamp to [0, dsp_rate / 2] while their gains differ (the reference's qsort
 * leaves their order undefined, eq.c:53-63; coinciding frequencies with equal gains are accepted). */
int qh_rxa_SetRXAEQRun(qh_rxa *e, int ch, int run);                             /* wdsp/eq.c:242-248 */
int qh_rxa_SetRXAEQNC(qh_rxa *e, int ch, int nc);                               /* wdsp/eq.c:250-265 */
int qh_rxa_SetRXAEQMP(qh_rxa *e, int ch, int mp);                               /* wdsp/eq.c:267-277 */
int qh_rxa_SetRXAEQProfile(qh_rxa *e, int ch, int nfreqs, const double *F, const double *G);   /* wdsp/eq.c:279-296 */
int qh_rxa_SetRXAEQCtfmode(qh_rxa *e, int ch, int mode);                        /* wdsp/eq.c:298-308 */
int qh_rxa_SetRXAEQWintype(qh_rxa *e, int ch, int wintype);                     /* wdsp/eq.c:310-320 */
int qh_rxa_SetRXAGrphEQ(qh_rxa *e, int ch, const int *rxeq);                    /* wdsp/eq.c:322-346: 4 values: preamp, then 150 and 400 Hz (both rxeq[1]), 1500, 6000 Hz; ctfmode 0 */
int qh_rxa_SetRXAGrphEQ10(qh_rxa *e, int ch, const int *rxeq);                  /* wdsp/eq.c:348-377: 11 values: preamp, then 32 ... 16000 Hz; ctfmode 0 */
int qh_rxa_SetRXAAMSQThreshold(qh_rxa *e, int ch, double threshold_db);
int qh_rxa_SetRXAAMSQMaxTail(qh_rxa *e, int ch, double tail_seconds);
/* xanf / xanr (wdsp/anf.c:82-133, anr.c:82-133), setters wdsp/anf.c:175-239 and anr.c:175-238; which position (0 before
 * bp1 and the AGC, 1 after the AGC) also moves bp1, as in the reference.  The reference's whole range runs: taps 1..2048 and
 * delay 0..2047 (ANF_DLINE_SIZE); a window that wraps the 2048-sample line (taps + delay > 2048) lands on the newest samples as it
 * does there.  Values outside are refused with QH_ERR_INVALID and change nothing. */
int qh_rxa_SetRXAANFRun(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANFTaps(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANFDelay(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANFPosition(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANFGain(qh_rxa *e, int ch, double v);
int qh_rxa_SetRXAANFLeakage(qh_rxa *e, int ch, double v);
int qh_rxa_SetRXAANFVals(qh_rxa *e, int ch, int taps, int delay, double gain, double leakage);
int qh_rxa_SetRXAANRRun(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANRTaps(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANRDelay(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANRPosition(qh_rxa *e, int ch, int v);
int qh_rxa_SetRXAANRGain(qh_rxa *e, int ch, double v);
int qh_rxa_SetRXAANRLeakage(qh_rxa *e, int ch, double v);
int qh_rxa_SetRXAANRVals(qh_rxa *e, int ch, int taps, int delay, double gain, double leakage);
/* The notch database and nbp0's notched band-pass (wdsp/nbp.c:358-525, make_nbp :97-179, fir_mbandpass :64-80).
 * *rval receives the reference's return value (0, or -1 for an index out of range). */
int qh_rxa_RXANBPAddNotch(qh_rxa *e, int ch, int notch, double fcenter, double fwidth, int active, int *rval);
int qh_rxa_RXANBPDeleteNotch(qh_rxa *e, int ch, int notch, int *rval);
int qh_rxa_RXANBPEditNotch(qh_rxa *e, int ch, int notch, double fcenter, double fwidth, int active, int *rval);
int qh_rxa_RXANBPGetNotch(qh_rxa *e, int ch, int notch, double *fcenter, double *fwidth, int *active, int *rval);
int qh_rxa_RXANBPGetNumNotches(qh_rxa *e, int ch, int *nnotches);
int qh_rxa_RXANBPGetMinNotchWidth(qh_rxa *e, int ch, double *minwidth);
int qh_rxa_RXANBPSetTuneFrequency(qh_rxa *e, int ch, double tunefreq);
int qh_rxa_RXANBPSetShiftFrequency(qh_rxa *e, int ch, double shift);
int qh_rxa_RXANBPSetNotchesRun(qh_rxa *e, int ch, int run);
int qh_rxa_RXANBPSetWindow(qh_rxa *e, int ch, int wintype);
int qh_rxa_RXANBPSetAutoIncrease(qh_rxa *e, int ch, int autoincr);
int qh_rxa_RXASetMP(qh_rxa *e, int ch, int mp);                  /* wdsp/RXA.c:948-958: minimum-phase filters (mp_imp, fir.c:319) in every fircore of the channel's chain */
/* nc, mp and window of nbp0, bpsnba and bp1, one setting per stage: RXASetNC / RXASetMP are these calls and the four FM, EQ and FMSQ ones
 * (RXA.c:934-958).  Each acts only on a value that changed.  A new nc zeroes that one stage's delay line (setNc_fircore, firmin.c:455-467)
 * and leaves every other stage's; a new mp or window designs the masks again and keeps the line (setMp_fircore, setImpulse_fircore).
 * Refused with QH_ERR_INVALID, nothing changed: an nc that is not a power of two in [dsp_size, 65536]; a window type other than 0 or 1. */
int qh_rxa_RXANBPSetNC(qh_rxa *e, int ch, int nc);                              /* wdsp/nbp.c:563-576 */
int qh_rxa_RXANBPSetMP(qh_rxa *e, int ch, int mp);                              /* wdsp/nbp.c:578-588 */
int qh_rxa_RXABPSNBASetNC(qh_rxa *e, int ch, int nc);                           /* wdsp/snb.c:829-842 */
int qh_rxa_RXABPSNBASetMP(qh_rxa *e, int ch, int mp);                           /* wdsp/snb.c:844-855 */
int qh_rxa_SetRXABandpassNC(qh_rxa *e, int ch, int nc);                         /* wdsp/bandpass.c:429-445 */
int qh_rxa_SetRXABandpassMP(qh_rxa *e, int ch, int mp);                         /* wdsp/bandpass.c:447-457 */
int qh_rxa_SetRXABandpassWindow(qh_rxa *e, int ch, int wintype);                /* wdsp/bandpass.c:411-427 */
int qh_rxa_SetRXAAMDFadeLevel(qh_rxa *e, int ch, int levelfade);
int qh_rxa_SetRXAFMDeviation(qh_rxa *e, int ch, double deviation);
int qh_rxa_SetRXACTCSSFreq(qh_rxa *e, int ch, double freq);
int qh_rxa_SetRXACTCSSRun(qh_rxa *e, int ch, int run);
/* xfmd's de-emphasis and audio filters (create_fmd's pde and paud, wdsp/fmd.c:110-118), every channel its own: nc max(2048, dsp_size) and
 * mp 0 for both, the audio band 300 .. 3000 Hz (RXA.c:196-197,209-212).  A setter acts only on a value that changed and takes effect at the
 * next process call.  SetRXAFMAFFilter and the two MP setters keep both filters' delay lines (setImpulse_fircore / setMp_fircore); an NC
 * setter zeroes the line of its own filter and leaves the other's (setNc_fircore, firmin.c:455-467).  RXASetNC and RXASetMP forward to the
 * four NC / MP setters of their channel (RXA.c:943-944,956-957).  The engine keeps one mask row per distinct design among its running FM
 * channels, so channels with equal settings share a row and, where the de-emphasis taps are real, a tile.
 * Refused by the setter with QH_ERR_INVALID, nothing changed (the reference checks none of this): an nc that is not a power of two in
 * [dsp_size, 65536]; a low or high that is not finite; low <= 0 (the de-emphasis design takes log10(high / low)); high <= low.
 * Refused with QH_ERR_UNSUPPORTED at the next process call while the channel's FM detector runs, nothing run: a band with
 * 1.1 * high >= dsp_rate / 2 (the audio filter's upper edge, fmd.c:115). */
int qh_rxa_SetRXAFMAFFilter(qh_rxa *e, int ch, double low, double high);        /* wdsp/fmd.c:364-384 */
int qh_rxa_SetRXAFMNCde(qh_rxa *e, int ch, int nc);                             /* wdsp/fmd.c:278-293 */
int qh_rxa_SetRXAFMMPde(qh_rxa *e, int ch, int mp);                             /* wdsp/fmd.c:295-305 */
int qh_rxa_SetRXAFMNCaud(qh_rxa *e, int ch, int nc);                            /* wdsp/fmd.c:307-322 */
int qh_rxa_SetRXAFMMPaud(qh_rxa *e, int ch, int mp);                            /* wdsp/fmd.c:324-334 */

/* Runs xrxa() (wdsp/RXA.c:561-598) over `nblk` consecutive DSP blocks of every channel.
 *   d_in  : device pointer, [nch][in_stride] interleaved complex double, nblk*dsp_insize samples used
 *   d_out : device pointer, [nch][out_stride] interleaved complex double, nblk*dsp_outsize samples written
 * Strides are in complex samples.  Filter/NCO state is carried to the next call exactly as the
 * reference carries it from block to block.  Asynchronous on the engine's stream.
 * The output rows may lie over the input rows (a caller that works in place): the engine then writes the output in a last pass
 * behind every read of the input instead of from its last filter's store -- the same samples within rounding (1e-11), decided by
 * the extent of the rows themselves (first sample of the first row to last sample of the last), not by where the matrices lie. */
int qh_rxa_process(qh_rxa *e, const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk);

/* Same with host buffers (synchronous; pageable memory; includes the PCIe copies).  h_out == h_in is allowed (rows of its own on the device). */
int qh_rxa_process_host(qh_rxa *e, const double *h_in, long long in_stride, double *h_out, long long out_stride, int nblk);

/* Tiles of the time-tiled FM loop that had to be re-run sequentially so far (diagnostics; 0 on carriers, a fraction of a
 * percent of the 256-sample tiles on noise alone). */
long long qh_rxa_pll_repairs(qh_rxa *h);
int qh_rxa_debug_pll(qh_rxa *h, int check_only, int ch, double *out, int max);   /* diagnostics, see qh_rxa_api.hip */
int qh_rxa_debug_fm_rows(qh_rxa *h, int *de_rows, int *aud_rows, long long *designed);   /* diagnostics: the design rows of xfmd's two filters on the device, and the rows designed on the host since the engine was made or rebuilt */
int qh_rxa_debug_fmsq(qh_rxa *h, int ch, double *out, int max);                      /* diagnostics: avnoise, longnoise, state, count, ready at the last call's end (wdsp/fmsq.c:141-205) */
int qh_rxa_debug_eqp(qh_rxa *h, int ch, double *taps, int max);                      /* diagnostics: returns nc and copies the complex taps behind the mask the channel's equalizer last got (2 nc doubles; a setter's design shows after the next process call that runs it); 0 while no channel of the engine has run the stage */
int qh_rxa_debug_agc(qh_rxa *h, int form);                                         /* diagnostics: 0 time tiles for long calls (default), 1 sample by sample, 2 batches of 64 */
int qh_rxa_debug_agc_ends(qh_rxa *h, int slot, double *out, int max);                /* diagnostics, see qh_rxa_api.hip */
long long qh_rxa_agc_repairs(qh_rxa *h);                                            /* wcpAGC time tiles the verify pass re-ran in order */
long long qh_rxa_agc_segments_rerun(qh_rxa *h);                                     /* super-segments of its boundary pass walked again */
int qh_rxa_agc_tiled_channels(qh_rxa *h);                                           /* channels whose xwcpagc took the time tiles in the last call */
int qh_rxa_synchronize(qh_rxa *e);

/* Meters (wdsp/meter.c:75-142).  They cost an extra pass, so they are off until enabled.  mt as wdsp/RXA.h:47-57:
 * 0 S_PK, 1 S_AV, 2 ADC_PK, 3 ADC_AV, 4 AGC_GAIN, 5 AGC_PK, 6 AGC_AV; values in dB, -400 before the first block. */
int qh_rxa_enable_meters(qh_rxa *e, int enable);
int qh_rxa_GetRXAMeter(qh_rxa *e, int ch, int mt, double *value);

/* The chain's two data taps: xsender behind nbp0 (wdsp/RXA.c:570) and xsiphon behind xwcpagc (wdsp/RXA.c:590).  Neither changes the
 * signal.  Both are OFF until enabled, per channel -- the reference runs the siphon of every channel (RXA.c:392-401): a tap costs a
 * pass, and a call with any tap on takes the per-mode path, as one with unfused meters does.  ch -1 = every channel.
 * Sender: later calls leave the channel's signal behind nbp0 as (I, Q) float pairs in engine-owned device rows, n samples of the last
 * call per row; rows of channels whose sender is off are not written.  Siphon: a ring of the newest 4096 samples (sipsize, RXA.c:392-401),
 * mode 0 only; get_sip returns the newest `size` complex samples, oldest first, zeros where fewer have arrived since the last flush.
 * Deviation: size < 0 or > 4096 returns QH_ERR_INVALID and leaves `out` alone (suck leaves sipout stale then, siphon.c:150, and
 * RXAGetaSipF reads `size` samples of it, past its end); a channel whose siphon is off is refused too.  It waits for the engine's stream. */
int qh_rxa_set_sender(qh_rxa *e, int ch, int run);                                 /* wdsp/sender.c:66-68 (run && flag) */
int qh_rxa_sender_rows(qh_rxa *e, const float **d_rows, long long *stride, int *n); /* wdsp/sender.c:75-80: [nch][stride] float pairs on the device */
int qh_rxa_sender_rows_host(qh_rxa *e, int ch, float *out, int max, int *n);        /* wdsp/sender.c:75-80: one channel's row, 2 n floats; waits */
int qh_rxa_set_siphon(qh_rxa *e, int ch, int run);                                 /* wdsp/siphon.c:96-130, mode 0; switched on, it starts flushed (siphon.c:88-94) */
int qh_rxa_get_sip(qh_rxa *e, int ch, double *out, int size);                      /* wdsp/siphon.c:148-163 (suck): 2 size doubles */

/* gen0, the signal generator at the head of xrxa (wdsp/gen.c:173-354, RXA.c:60-66,565).  A channel whose generator runs has its buffer
 * behind xshift / xresample REPLACED by the generated signal (both still run and keep their state; the call's input is not looked at
 * otherwise): the adc meter, the notched band-pass and everything behind them see the generator.  Created with run 0, mode 2, as create_rxa
 * does.  Modes: 0 tone, 1 two tones (0.5 / 0.5 at 900 / 1700 Hz, no RXA setter), 2 noise, 3 sweep, 6 a keyed 1 kHz pulse (0.25 Hz, duty
 * 0.25, 2 ms edges, no RXA setter), any other silence.  Every mode keeps its own state and only the running mode's moves.  ch -1 = every
 * channel.  Deviations: modes 4 and 5 (sawtooth, triangle: "audio only", no RXA setter) are refused while the generator runs -- the next
 * process call returns QH_ERR_UNSUPPORTED and runs nothing; the noise is the reference's polar method on a counter-based source keyed by
 * (seed, channel, sample), not rand() seeded by the clock and shared by the process; a sweep whose period exceeds 2^27 samples resets at
 * the closed form's instants, not the addition chain's. */
int qh_rxa_SetRXAPreGenRun(qh_rxa *e, int ch, int run);                            /* wdsp/gen.c:384-390 */
int qh_rxa_SetRXAPreGenMode(qh_rxa *e, int ch, int mode);                          /* wdsp/gen.c:392-398 */
int qh_rxa_SetRXAPreGenToneMag(qh_rxa *e, int ch, double mag);                     /* wdsp/gen.c:400-406 */
int qh_rxa_SetRXAPreGenToneFreq(qh_rxa *e, int ch, double freq);                   /* wdsp/gen.c:408-415: the phase goes to 0 (calc_tone) */
int qh_rxa_SetRXAPreGenNoiseMag(qh_rxa *e, int ch, double mag);                    /* wdsp/gen.c:417-423 */
int qh_rxa_SetRXAPreGenSweepMag(qh_rxa *e, int ch, double mag);                    /* wdsp/gen.c:425-431 */
int qh_rxa_SetRXAPreGenSweepFreq(qh_rxa *e, int ch, double freq1, double freq2);   /* wdsp/gen.c:433-441: the sweep starts again (calc_sweep) */
int qh_rxa_SetRXAPreGenSweepRate(qh_rxa *e, int ch, double rate);                  /* wdsp/gen.c:443-450: the sweep starts again (calc_sweep) */
int qh_rxa_set_gen_seed(qh_rxa *e, int ch, unsigned long long seed);               /* wdsp/gen.c:131 (srand): the noise stream's seed; default: a fixed function of ch */

/* flush_rxa (wdsp/RXA.c:527-559): zero the NCO phase and every filter history of every channel. */
int qh_rxa_flush(qh_rxa *e);

/* Timing of the kernels of qh_rxa_process with HIP events on the engine's stream.
 * enable != 0 brackets every kernel of later process calls with events; qh_rxa_timing() waits for
 * the last call and returns, for kernel k (0 = shift+resample stage, 1 = bandpass stage, 2 = state
 * bookkeeping), the milliseconds of the last call in ms[k].  Returns the number of entries. */
int qh_rxa_enable_timing(qh_rxa *e, int enable);
int qh_rxa_timing(qh_rxa *e, double *ms, int n);

/* Bytes of device memory the engine holds: the sum of its own live device allocations (state, masks,
 * channel lists, intermediate buffers).  The qh_rat resamplers behind it (in_rate or out_rate ratios
 * the overlap-save stages do not cover) keep their own memory and are not included. */
long long qh_rxa_device_bytes(const qh_rxa *e);

/* The run-time rate and buffer-size setters of wdsp/channel.c:169-258 on a live engine.  Every per-channel setting survives; a call that
 * changes nothing does nothing (channel.c's `if (x != ch[channel].x)`: the captured launch sequences stay too); a value qh_rxa_create
 * would refuse, a dsp_size above a channel's nc (nbp.c:308) or a dsp_size change under an attached display is refused with create's
 * status and changes nothing.  What each change does to each stage's state follows setInputSamplerate_rxa ... setDSPBuffsize_rxa
 * (wdsp/RXA.c:600-740), tabled in DESIGN.md row b24: a new in_rate restarts the shift at phase 0 and makes rsmpin anew, a new out_rate
 * makes rsmpout anew -- both leave everything at the DSP rate running; a new dsp_rate or dsp_size starts every stage from zero, except
 * what the reference keeps: anf / anr's lidx and ngamma and snba's frame memory (both changes); the delay lines of nbp0, bp1, eqp and
 * xfmd's filters (nc <= 4096) and the SAM detector's sideband chains (a new dsp_rate); the whole AM / SAM detector and gen0's phases and
 * positions, its pulse flushed (a new dsp_size).
 * qh_rxa_dsp_insize / _outsize and qh_rxa_device_bytes follow. */
int qh_rxa_set_rates(qh_rxa *e, int in_rate, int dsp_rate, int out_rate);    /* SetAllRates, wdsp/channel.c:242-258 */
int qh_rxa_set_in_rate(qh_rxa *e, int in_rate);                              /* SetInputSamplerate, wdsp/channel.c:198-210 + RXA.c:600-614 */
int qh_rxa_set_dsp_rate(qh_rxa *e, int dsp_rate);                            /* SetDSPSamplerate, wdsp/channel.c:212-226 + RXA.c:627-671 */
int qh_rxa_set_out_rate(qh_rxa *e, int out_rate);                            /* SetOutputSamplerate, wdsp/channel.c:228-240 + RXA.c:616-625 */
int qh_rxa_set_dsp_size(qh_rxa *e, int dsp_size);                            /* SetDSPBuffsize, wdsp/channel.c:182-196 + RXA.c:673-740 */
int qh_rxa_in_rate(const qh_rxa *e);                                         /* ch[].in_rate, wdsp/channel.c:81 */
int qh_rxa_dsp_rate(const qh_rxa *e);                                        /* ch[].dsp_rate, wdsp/channel.c:82 */
int qh_rxa_out_rate(const qh_rxa *e);                                        /* ch[].out_rate, wdsp/channel.c:83 */
int qh_rxa_dsp_size(const qh_rxa *e);                                        /* ch[].dsp_size, wdsp/channel.c:80 */

/* ------------------------------------------------------------------ 2. WDSP drop-in exports */
/* Signatures are the reference's: wdsp/channel.h:62, wdsp/iobuffs.h:89-90, and the PORT functions
 * cited per line.  Channel numbers 0..31 (wdsp/comm.h:117).  Each open channel is a 1-channel
 * qh_rxa engine plus the host-side ring logic of wdsp/iobuffs.c (two-block latency, upslew). */
int GetWDSPVersion(void);                                                        /* wdsp/version.c */
void OpenChannel(int channel, int in_size, int dsp_size, int input_samplerate, int dsp_rate,
                 int output_samplerate, int type, int state, double tdelayup, double tslewup,
                 double tdelaydown, double tslewdown, int bfo);                  /* wdsp/channel.c:75-103 */
void CloseChannel(int channel);                                                  /* wdsp/channel.c:122-128 */
int SetChannelState(int channel, int state, int dmode);                          /* wdsp/channel.c:260-298 */
/* The channel's run-time setters.  Each rebuilds the iobuffs as pre_main_destroy / post_main_destroy / pre_main_build do (out_size, the
 * rings as create_iobuffs leaves them, the slews from the stored times at the new rates, the staging; samples in flight are lost) and
 * hands the engine its part (qh_rxa_set_*).  SetDSPBuffsize and SetDSPSamplerate bracket the change with SetChannelState(channel, 0, 1)
 * and SetChannelState(channel, old, 0): a channel that was running has its up-slew armed again; the others arm nothing.  A value the
 * engine refuses (qh_rxa_set_rates), an in_size <= 0 or a channel that is not open sets qh_wdsp_status() and changes nothing.  SetType:
 * type 0 does nothing, any other type is refused (QH_ERR_UNSUPPORTED) as OpenChannel does.  The re-blocking shim (wdspFexchange0) holds
 * its own in_size (qh_wdsp_set_parameter) and its ring, on the host or the device, is sized by that: SetInputBuffsize does not touch it,
 * and qh_wdsp_fexchange0_device refuses to run while the two sizes differ -- give the shim the new size with qh_wdsp_set_parameter. */
void SetType(int channel, int type);                                             /* wdsp/channel.c:158-167 */
void SetInputBuffsize(int channel, int in_size);                                 /* wdsp/channel.c:169-180 */
void SetDSPBuffsize(int channel, int dsp_size);                                  /* wdsp/channel.c:182-196 */
void SetInputSamplerate(int channel, int samplerate);                            /* wdsp/channel.c:198-210 */
void SetDSPSamplerate(int channel, int samplerate);                              /* wdsp/channel.c:212-226 */
void SetOutputSamplerate(int channel, int samplerate);                           /* wdsp/channel.c:228-240 */
void SetAllRates(int channel, int in_rate, int dsp_rate, int out_rate);          /* wdsp/channel.c:242-258 */
void SetChannelTDelayUp(int channel, double time);                               /* wdsp/channel.c:301-311: flush_slews */
void SetChannelTSlewUp(int channel, double time);                                /* wdsp/channel.c:313-323: the slews are made anew */
void SetChannelTDelayDown(int channel, double time);                             /* wdsp/channel.c:325-335: flush_slews */
void SetChannelTSlewDown(int channel, double time);                              /* wdsp/channel.c:337-347: the slews are made anew */
void fexchange0(int channel, double *in, double *out, int *error);               /* wdsp/iobuffs.c:464-516 */
void fexchange2(int channel, float *Iin, float *Qin, float *Iout, float *Qout, int *error);     /* wdsp/iobuffs.c:518-582 */
void SetRXAMode(int channel, int mode);                                          /* wdsp/RXA.c:748-787 */
void RXASetPassband(int channel, double f_low, double f_high);                   /* wdsp/RXA.c:926-932 */
void RXASetNC(int channel, int nc);                                              /* wdsp/RXA.c:934-946 */
void RXASetMP(int channel, int mp);                                              /* wdsp/RXA.c:948-958 */
void SetRXAShiftRun(int channel, int run);                                       /* wdsp/shift.c:110-117 */
void SetRXAShiftFreq(int channel, double fshift);                                /* wdsp/shift.c:119-127 */
void RXANBPSetRun(int channel, int run);                                         /* wdsp/nbp.c:528-536 */
void RXANBPSetFreqs(int channel, double flow, double fhigh);                     /* wdsp/nbp.c:538-552 */
void SetRXABandpassRun(int channel, int run);                                    /* wdsp/bandpass.c:381-387 */
void SetRXABandpassFreqs(int channel, double f_low, double f_high);              /* wdsp/bandpass.c:389-407 */
void SetRXAAGCMode(int channel, int mode);                                       /* wdsp/wcpAGC.c:369-411 */
void SetRXAAGCFixed(int channel, double fixed_agc);                              /* wdsp/wcpAGC.c:541-548 */
void SetRXAAGCAttack(int channel, int attack);                                   /* wdsp/wcpAGC.c:413-420 */
void SetRXAAGCDecay(int channel, int decay);                                     /* wdsp/wcpAGC.c:422-429 */
void SetRXAAGCHang(int channel, int hang);                                       /* wdsp/wcpAGC.c:431-438 */
void SetRXAAGCTop(int channel, double max_agc);                                  /* wdsp/wcpAGC.c:520-527 */
void SetRXAAGCSlope(int channel, int slope);                                     /* wdsp/wcpAGC.c:529-536 */
void SetRXAAGCHangThreshold(int channel, int hangthreshold);                     /* wdsp/wcpAGC.c:480-487 */
void SetRXAPanelRun(int channel, int run);                                       /* wdsp/patchpanel.c:123-129 */
void SetRXAPanelGain1(int channel, double gain);                                 /* wdsp/patchpanel.c:139-145 */
void SetRXAPanelGain2(int channel, double gainI, double gainQ);                  /* wdsp/patchpanel.c:147-154 */
void SetRXAPanelSelect(int channel, int select);                                 /* wdsp/patchpanel.c:131-137 */
void SetRXAPanelCopy(int channel, int copy);                                     /* wdsp/patchpanel.c:175-181 */
void SetRXAPanelPan(int channel, double pan);                                    /* wdsp/patchpanel.c:158-176 */
void SetRXAPanelBinaural(int channel, int bin);                                  /* wdsp/patchpanel.c:186-192 */
/* (the refusals of the qh_rxa_* forms above set qh_wdsp_status(); a getter of a channel that is not open leaves its result alone) */
void SetRXAAGCThresh(int channel, double thresh, double size, double rate);      /* wdsp/wcpAGC.c:499-511 */
void GetRXAAGCThresh(int channel, double *thresh, double size, double rate);     /* wdsp/wcpAGC.c:487-497 */
void SetRXAAGCHangLevel(int channel, double hangLevel);                          /* wdsp/wcpAGC.c:449-466 */
void GetRXAAGCHangLevel(int channel, double *hangLevel);                         /* wdsp/wcpAGC.c:440-447 */
void GetRXAAGCHangThreshold(int channel, int *hangthreshold);                    /* wdsp/wcpAGC.c:468-475 */
void GetRXAAGCTop(int channel, double *max_agc);                                 /* wdsp/wcpAGC.c:513-520 */
void SetRXAAGCMaxInputLevel(int channel, double level);                          /* wdsp/wcpAGC.c:550-557 */
void RXANBPSetNC(int channel, int nc);                                           /* wdsp/nbp.c:563-576 */
void RXANBPSetMP(int channel, int mp);                                           /* wdsp/nbp.c:578-588 */
void RXABPSNBASetNC(int channel, int nc);                                        /* wdsp/snb.c:829-842 */
void RXABPSNBASetMP(int channel, int mp);                                        /* wdsp/snb.c:844-855 */
void SetRXABandpassNC(int channel, int nc);                                      /* wdsp/bandpass.c:429-445 */
void SetRXABandpassMP(int channel, int mp);                                      /* wdsp/bandpass.c:447-457 */
void SetRXABandpassWindow(int channel, int wintype);                             /* wdsp/bandpass.c:411-427 */
/* There are no FFTW plans to make here: WDSPwisdom returns at once, as the reference does when its wisdom file already exists (it touches
 * no file and ignores a null or unwritable directory), and the status string stays the empty one the reference has in that case. */
void WDSPwisdom(char *directory);                                                /* wdsp/wisdom.c:38-121 */
char *wisdom_get_status(void);                                                   /* wdsp/wisdom.c:32-36: a static, NUL-terminated string */
void SetRXAAMDSBMode(int channel, int sbmode);                                   /* wdsp/amd.c:277-283 */
void SetRXAAMDRun(int channel, int run);                                         /* wdsp/amd.c:264-277 */
void SetRXAFMLimRun(int channel, int run);                                       /* wdsp/fmd.c:336-347 */
void SetRXAFMLimGain(int channel, double gaindB);                                /* wdsp/fmd.c:349-362 */
int RXANBPAddNotch(int channel, int notch, double fcenter, double fwidth, int active);          /* wdsp/nbp.c:358-388 */
int RXANBPGetNotch(int channel, int notch, double *fcenter, double *fwidth, int *active);       /* wdsp/nbp.c:390-412 */
int RXANBPDeleteNotch(int channel, int notch);                                   /* wdsp/nbp.c:414-438 */
int RXANBPEditNotch(int channel, int notch, double fcenter, double fwidth, int active);         /* wdsp/nbp.c:440-459 */
void RXANBPGetNumNotches(int channel, int *nnotches);                            /* wdsp/nbp.c:461-469 */
void RXANBPSetTuneFrequency(int channel, double tunefreq);                       /* wdsp/nbp.c:471-481 */
void RXANBPSetShiftFrequency(int channel, double shift);                         /* wdsp/nbp.c:483-493 */
void RXANBPSetNotchesRun(int channel, int run);                                  /* wdsp/nbp.c:495-514 */
void RXANBPSetWindow(int channel, int wintype);                                  /* wdsp/nbp.c:542-560 */
void RXANBPSetAutoIncrease(int channel, int autoincr);                           /* wdsp/nbp.c:600-619 */
void RXANBPGetMinNotchWidth(int channel, double *minwidth);                      /* wdsp/nbp.c:588-597 */
void SetRXAAMDFadeLevel(int channel, int levelfade);                             /* wdsp/amd.c:285-291 */
void SetRXAFMDeviation(int channel, double deviation);                           /* wdsp/fmd.c:236-246 */
void SetRXACTCSSFreq(int channel, double freq);                                  /* wdsp/fmd.c:248-258 */
void SetRXACTCSSRun(int channel, int run);                                       /* wdsp/fmd.c:260-267 */
void SetRXAFMAFFilter(int channel, double low, double high);                     /* wdsp/fmd.c:364-384 */
void SetRXAFMNCde(int channel, int nc);                                          /* wdsp/fmd.c:278-293 */
void SetRXAFMMPde(int channel, int mp);                                          /* wdsp/fmd.c:295-305 */
void SetRXAFMNCaud(int channel, int nc);                                         /* wdsp/fmd.c:307-322 */
void SetRXAFMMPaud(int channel, int mp);                                         /* wdsp/fmd.c:324-334 */
double GetRXAMeter(int channel, int mt);                                         /* wdsp/meter.c:133-142 */
/* gen0 (see qh_rxa_SetRXAPreGenRun).  SetRXAPreGenMode 4 or 5 while the generator runs: the next fexchange0 sets qh_wdsp_status() and leaves
 * its output buffer alone. */
void SetRXAPreGenRun(int channel, int run);                                      /* wdsp/gen.c:384-390 */
void SetRXAPreGenMode(int channel, int mode);                                    /* wdsp/gen.c:392-398 */
void SetRXAPreGenToneMag(int channel, double mag);                               /* wdsp/gen.c:400-406 */
void SetRXAPreGenToneFreq(int channel, double freq);                             /* wdsp/gen.c:408-415 */
void SetRXAPreGenNoiseMag(int channel, double mag);                              /* wdsp/gen.c:417-423 */
void SetRXAPreGenSweepMag(int channel, double mag);                              /* wdsp/gen.c:425-431 */
void SetRXAPreGenSweepFreq(int channel, double freq1, double freq2);             /* wdsp/gen.c:433-441 */
void SetRXAPreGenSweepRate(int channel, double rate);                            /* wdsp/gen.c:443-450 */
/* The sender runs on channel 0 only, as create_rxa makes it (RXA.c:131): on another channel the call is accepted and does nothing.  With
 * flag set, every DSP block of channel 0 feeds display `disp` (XCreateAnalyzer), sub-span ss, on the device; the display is looked up at
 * each block, and one that does not exist or whose buff_size is not dsp_size sets qh_wdsp_status() and is fed nothing.  The siphon is off
 * until a channel's first RXAGetaSipF / RXAGetaSipF1 call, which switches it on and returns a flushed siphon's zeros (deviation: the
 * reference runs it from create_rxa on); size outside 0 .. 4096 sets qh_wdsp_status() and leaves `out` alone. */
void SetRXASpectrum(int channel, int flag, int disp, int ss, int LO);           /* wdsp/sender.c:111-122 */
void RXAGetaSipF(int channel, float *out, int size);                            /* wdsp/siphon.c:182-195: I only */
void RXAGetaSipF1(int channel, float *out, int size);                           /* wdsp/siphon.c:197-211: I, Q */
/* The blanker WDSP's callers run in front of fexchange0 (wdsp/nob.c:307-422, wdsp.h:620-665): ids 0..31, each a one-channel qh_anb bank
 * with staging rows of its own, so in == out works as it does for the reference's callers; buffsize is the n of xanbEXT.  in / out
 * are host pointers, as fexchange0's are; samples that are already on the GPU go through qh_wdsp_xanbEXT_device, as fexchange0's go
 * through qh_wdsp_fexchange0_device.  Errors (a bad or empty id, a refused value: see qh_anb_create) go to qh_wdsp_status() and change
 * nothing.  Not provided: xanbEXTF and the "legacy interface" (nob.c:424-448), the pointer-based pSetRCVRANB* (nob.c:226-299). */
void create_anbEXT(int id, int run, int buffsize, double samplerate, double tau, double hangtime, double advtime, double backtau,
                   double threshold);                                            /* wdsp/nob.c:310-324 */
void destroy_anbEXT(int id);                                                     /* wdsp/nob.c:326-330 */
void flush_anbEXT(int id);                                                       /* wdsp/nob.c:332-336 */
void xanbEXT(int id, double *in, double *out);                                   /* wdsp/nob.c:338-345 */
void SetEXTANBRun(int id, int run);                                              /* wdsp/nob.c:347-354 */
void SetEXTANBBuffsize(int id, int size);                                        /* wdsp/nob.c:356-363 */
void SetEXTANBSamplerate(int id, int rate);                                      /* wdsp/nob.c:365-373 */
void SetEXTANBTau(int id, double tau);                                           /* wdsp/nob.c:375-383 */
void SetEXTANBHangtime(int id, double time);                                     /* wdsp/nob.c:385-393 */
void SetEXTANBAdvtime(int id, double time);                                      /* wdsp/nob.c:395-403 */
void SetEXTANBBacktau(int id, double tau);                                       /* wdsp/nob.c:405-413 */
void SetEXTANBThreshold(int id, double thresh);                                  /* wdsp/nob.c:415-422 */
/* xanbEXT for buffsize samples in device memory (d_in == d_out allowed): enqueued on the id's stream, which is ordered behind `stream`
 * on entry; `stream` is ordered behind it on return.  Nothing is waited for.  The same samples as xanbEXT, bit for bit. */
int qh_wdsp_xanbEXT_device(int id, const void *d_in, void *d_out, void *stream);
/* WDSP's second blanker, the callers' "NB2" (wdsp/nobII.c:605-734): ids 0..31, each a one-channel qh_nob bank with staging rows of its
 * own, so in == out works; buffsize is the n of xnobEXT.  slewtime is both the advance and the hang slew time and max_imp_seq_time is
 * 0.025 s, as create_nobEXT fixes them (nobII.c:622-624).  Errors (a bad or empty id, a refused value: see qh_nob_create) go to
 * qh_wdsp_status() and change nothing.  Not provided: xnobEXTF and the "legacy interface" (nobII.c:742-760), the pointer-based
 * pSetRCVRNOB* (nobII.c:521-597). */
void create_nobEXT(int id, int run, int mode, int buffsize, double samplerate, double slewtime, double hangtime, double advtime,
                   double backtau, double threshold);                            /* wdsp/nobII.c:608-626 */
void destroy_nobEXT(int id);                                                     /* wdsp/nobII.c:628-632 */
void flush_nobEXT(int id);                                                       /* wdsp/nobII.c:634-638 */
void xnobEXT(int id, double *in, double *out);                                   /* wdsp/nobII.c:640-647 */
void SetEXTNOBRun(int id, int run);                                              /* wdsp/nobII.c:649-656 */
void SetEXTNOBMode(int id, int mode);                                            /* wdsp/nobII.c:658-665 */
void SetEXTNOBBuffsize(int id, int size);                                        /* wdsp/nobII.c:667-674 */
void SetEXTNOBSamplerate(int id, int rate);                                      /* wdsp/nobII.c:676-684 */
void SetEXTNOBTau(int id, double tau);                                           /* wdsp/nobII.c:686-695 */
void SetEXTNOBHangtime(int id, double time);                                     /* wdsp/nobII.c:697-705 */
void SetEXTNOBAdvtime(int id, double time);                                      /* wdsp/nobII.c:707-715 */
void SetEXTNOBBacktau(int id, double tau);                                       /* wdsp/nobII.c:717-725 */
void SetEXTNOBThreshold(int id, double thresh);                                  /* wdsp/nobII.c:727-734 */
/* xnobEXT for buffsize samples in device memory (d_in == d_out allowed): enqueued on the id's stream, which is ordered behind `stream`
 * on entry; `stream` is ordered behind it on return.  Nothing is waited for.  The same samples as xnobEXT, bit for bit. */
int qh_wdsp_xnobEXT_device(int id, const void *d_in, void *d_out, void *stream);
/* The diversity combiner WDSP's callers run behind the blankers and in front of fexchange0 (wdsp/div.c:104-187): ids 0..31 (WDSP's own
 * array holds 2, MAX_EXT_DIVS, div.c:104), each a one-group qh_div bank (section 10e) with staging rows of its own.  xdivEXT takes
 * nsamples as the size and the first nr pointers of `in`; in[i] and out are host pointers.  out == in[k] is recognised by pointer
 * equality and gives what the reference gives: in the mixing mode every receiver whose pointer is `out` contributes the running sum in
 * place of its samples (the memset has zeroed them, div.c:81), and a copy of in[output] onto itself does nothing.  Refused, to
 * qh_wdsp_status() with nothing changed: a bad or empty id; a null pointer among those the call reads (in, out, in[i] of the receivers
 * it reads); any other overlap of out with an input that is read; nsamples < 0; output > nr while the id runs; nr outside 1..8,
 * output outside 0..8, SetEXTDIVRotate's nr outside 0..8, a null or non-finite rotate array (the reference reads a stale or null pointer
 * or writes past Irotate[8] there).  SetEXTDIVBuffsize stores the size (a negative one is refused); xdivEXT's nsamples is what counts,
 * as in the reference.  flush_divEXT does nothing, as there.  The setters are order-free and act on the next xdivEXT.
 * Not provided: xdivEXTF and the "legacy interface" (div.c:189-219). */
void create_divEXT(int id, int run, int nr, int size);                           /* wdsp/div.c:107-111: output 0, rotates 0 */
void destroy_divEXT(int id);                                                     /* wdsp/div.c:113-117 */
void flush_divEXT(int id);                                                       /* wdsp/div.c:119-123 */
void xdivEXT(int id, int nsamples, double **in, double *out);                    /* wdsp/div.c:125-134 */
void SetEXTDIVRun(int id, int run);                                              /* wdsp/div.c:137-144 */
void SetEXTDIVBuffsize(int id, int size);                                        /* wdsp/div.c:147-154 */
void SetEXTDIVNr(int id, int nr);                                                /* wdsp/div.c:157-164 */
void SetEXTDIVOutput(int id, int output);                                        /* wdsp/div.c:168-175 */
void SetEXTDIVRotate(int id, int nr, double *Irotate, double *Qrotate);          /* wdsp/div.c:179-187 */
/* xdivEXT for nsamples samples in device memory: d_in is a host array of nr device pointers, read before the call returns; d_out ==
 * d_in[k] is recognised as in xdivEXT.  Enqueued on the id's stream, which is ordered behind `stream` on entry; `stream` is ordered
 * behind it on return.  Nothing is waited for.  The same samples as xdivEXT, bit for bit.  The rows the call reads are gathered into
 * the id's staging rows first (one device copy each); a caller whose receivers already lie in strided rows uses qh_div_process. */
int qh_wdsp_xdivEXT_device(int id, int nsamples, const void *const *d_in, void *d_out, void *stream);
/* The variable-ratio resampler WDSP's callers put behind fexchange0 (wdsp/varsamp.c:228-250): every pointer a one-channel qh_varsamp
 * bank (section 10d) with run 1, fc 0, fc_low -1, gain 1, var 1 and varmode 1, as create_varsampV fixes them, on a stream and with an
 * input staging row of its own, so input == output works.  input / output are host pointers; output needs room for the samples the
 * call makes (about numsamps * var * out_rate / in_rate, at most qh_wdsp_varsampV_max_out), as the reference's does.  Errors (a
 * pointer that create_varsampV did not return, a refused value: see qh_varsamp_create) go to qh_wdsp_status(), change nothing and
 * report *outsamps = 0; create_varsampV then returns null.  Not provided: rmatch.c (create_rmatchV, xrmatchIN, xrmatchOUT ...), which
 * is host threading around this call. */
void *create_varsampV(int in_rate, int out_rate, int R);                         /* wdsp/varsamp.c:230-234 */
void xvarsampV(double *input, double *output, int numsamps, double var, int *outsamps, void *ptr);  /* wdsp/varsamp.c:236-244 */
void destroy_varsampV(void *ptr);                                                /* wdsp/varsamp.c:246-250 */
long long qh_wdsp_varsampV_max_out(void *ptr, int numsamps, double var);         /* qh_varsamp_max_out of the pointer's bank */
/* xvarsampV for numsamps samples in device memory (d_in == d_out allowed; d_out with room for qh_wdsp_varsampV_max_out samples;
 * d_count: device, one int): enqueued on the pointer's stream, which is ordered behind `stream` on entry; `stream` is ordered behind
 * it on return.  Nothing is waited for.  The same samples and count as xvarsampV, bit for bit. */
int qh_wdsp_xvarsampV_device(void *ptr, const void *d_in, void *d_out, int numsamps, double var, int *d_count, void *stream);
/* The fixed-ratio resampler WDSP's callers use beside fexchange0 (wdsp/resample.c:206-228, 332-354): every pointer a one-channel
 * qh_resample bank (section 10f) on a stream and with staging rows of its own -- complex doubles with run 1, fc 0, ncoef 0 and gain 1
 * for the V names, real floats for the FV names -- looked up in a table, not followed.  *outsamps is the number of samples the call
 * makes (ceil((numsamps L - phnum) / M), at most qh_wdsp_resampleV_max_out), as the reference's is.  input == output works where
 * L <= M and gives the reference's result there (it never reads a sample it has overwritten); where L > M the reference overwrites
 * samples it has yet to read, and the call is refused.  Errors (a pointer that create did not return, a refused rate pair: see
 * qh_resample_create, input == output with L > M) go to qh_wdsp_status(), change nothing and report *outsamps = 0; create then returns
 * null.  Not provided: create_resample, destroy_resample, flush_resample, xresample and the set..._resample names, whose argument is
 * WDSP's own struct; qh_resample_* has their function. */
void *create_resampleV(int in_rate, int out_rate);                                /* wdsp/resample.c:208-212 */
void xresampleV(double *input, double *output, int numsamps, int *outsamps, void *ptr);   /* wdsp/resample.c:214-222 */
void destroy_resampleV(void *ptr);                                                /* wdsp/resample.c:224-228 */
void *create_resampleFV(int in_rate, int out_rate);                               /* wdsp/resample.c:334-338 */
void xresampleFV(float *input, float *output, int numsamps, int *outsamps, void *ptr);    /* wdsp/resample.c:340-348 */
void destroy_resampleFV(void *ptr);                                               /* wdsp/resample.c:350-354 */
long long qh_wdsp_resampleV_max_out(void *ptr, int numsamps);                     /* qh_resample_max_out of a V or FV pointer's bank */
/* xresampleV / xresampleFV for numsamps samples in device memory (d_out with room for qh_wdsp_resampleV_max_out samples; d_in ==
 * d_out as above; *outsamps: host, set before the call returns): enqueued on the pointer's stream, which is ordered behind `stream` on
 * entry; `stream` is ordered behind it on return.  Nothing is waited for.  The same samples and count as the host forms, bit for bit. */
int qh_wdsp_xresampleV_device(void *ptr, const void *d_in, void *d_out, int numsamps, int *outsamps, void *stream);
int qh_wdsp_xresampleFV_device(void *ptr, const void *d_in, void *d_out, int numsamps, int *outsamps, void *stream);
/* Quisk's re-blocking shim around fexchange0 (quisk_wdsp.c:24-69): any nSamples in, scaled by 1/CLIP32 into
 * in_size blocks, results scaled back; returns the number of samples written to cSamples.  qh_wdsp_set_parameter
 * is the C form of quisk_wdsp_set_parameter (quisk_wdsp.c:71-91; in_size <= 0 / in_use < 0 leave the value).  One deviation: a CHANGE
 * of in_size starts the ring again -- the reference keeps a ring whose length is no longer a multiple of the block and reads past
 * its end (quisk_wdsp.c:44-49,57-60). */
int wdspFexchange0(int channel, double *cSamples, int nSamples);
void qh_wdsp_set_parameter(int channel, int in_size, int in_use);
/* The same hand-off for samples that are already on the GPU (what qh_quisk_process_samples does at quisk.c:2660-2661):
 * d_samples = nSamples interleaved complex doubles in device memory with room for nSamples + in_size; the shim's ring, the
 * double rings of fexchange0 (wdsp/iobuffs.c:464-516), the up- and down-slews and the DSP blocks all stay in device memory
 * and are enqueued on the channel's stream (ordered behind `stream` on entry; `stream` is ordered behind it on return) --
 * no copy to the host, nothing waited for.  Returns the number of samples left in d_samples, like wdspFexchange0.  The same
 * samples as the host-pointer call, bit for bit; a channel may change between the two in mid-stream. */
int qh_wdsp_fexchange0_device(int channel, void *d_samples, int nSamples, void *stream);
/* accepted and ignored: these blocks are run = 0 on the hot path */
/* anf / anr: the leaky-LMS automatic notch filter and noise reduction of the RXA chain (wdsp/anf.c:175-239, anr.c:175-238);
 * taps 1..2048 and delay 0..2047, the reference's delay line (defaults 64 / 16, RXA.c:285-286,305-306); a value outside is refused,
 * nothing changes and qh_wdsp_status() says so */
void SetRXAANFRun(int channel, int v);
void SetRXAANFTaps(int channel, int v);
void SetRXAANFDelay(int channel, int v);
void SetRXAANFPosition(int channel, int v);
void SetRXAANFGain(int channel, double v);
void SetRXAANFLeakage(int channel, double v);
void SetRXAANFVals(int channel, int taps, int delay, double gain, double leakage);
void SetRXAANRRun(int channel, int v);
void SetRXAANRTaps(int channel, int v);
void SetRXAANRDelay(int channel, int v);
void SetRXAANRPosition(int channel, int v);
void SetRXAANRGain(int channel, double v);
void SetRXAANRLeakage(int channel, double v);
void SetRXAANRVals(int channel, int taps, int delay, double gain, double leakage);
void SetRXAAMSQRun(int channel, int run);                                        /* wdsp/amsq.c:216-222 */
void SetRXACBLRun(int channel, int setit);                                       /* wdsp/cblock.c:120-126, wdsp.h:277 */
void SetRXASPCWRun(int channel, int run);                                        /* wdsp/iir.c:322-360, wdsp.h:557-560 */
void SetRXASPCWFreq(int channel, double freq);
void SetRXASPCWBandwidth(int channel, double bw);
void SetRXASPCWGain(int channel, double gain);
void SetRXAmpeakRun(int channel, int run);                                       /* wdsp/iir.c:490-548, wdsp.h:561-566 */
void SetRXAmpeakNpeaks(int channel, int npeaks);
void SetRXAmpeakFilEnable(int channel, int fil, int enable);
void SetRXAmpeakFilFreq(int channel, int fil, double freq);
void SetRXAmpeakFilBw(int channel, int fil, double bw);
void SetRXAmpeakFilGain(int channel, int fil, double gain);
void SetRXASSQLRun(int channel, int run);                                        /* wdsp/ssql.c:330-336 */
void SetRXASSQLThreshold(int channel, double threshold);                         /* wdsp/ssql.c:338-346 */
void SetRXASSQLTauMute(int channel, double tau_mute);                            /* wdsp/ssql.c:348-358 */
void SetRXASSQLTauUnMute(int channel, double tau_unmute);                        /* wdsp/ssql.c:360-370 */
void SetRXAFMSQRun(int channel, int run);                                        /* wdsp/fmsq.c:235-241 */
void SetRXAFMSQThreshold(int channel, double threshold);                         /* wdsp/fmsq.c:243-250 */
void SetRXAFMSQNC(int channel, int nc);                                          /* wdsp/fmsq.c:252-267 */
void SetRXAFMSQMP(int channel, int mp);                                          /* wdsp/fmsq.c:269-279 */
void SetRXAEQRun(int channel, int run);                                          /* wdsp/eq.c:242-248 */
void SetRXAEQNC(int channel, int nc);                                            /* wdsp/eq.c:250-265 */
void SetRXAEQMP(int channel, int mp);                                            /* wdsp/eq.c:267-277 */
void SetRXAEQProfile(int channel, int nfreqs, double *F, double *G);             /* wdsp/eq.c:279-296 */
void SetRXAEQCtfmode(int channel, int mode);                                     /* wdsp/eq.c:298-308 */
void SetRXAEQWintype(int channel, int wintype);                                  /* wdsp/eq.c:310-320 */
void SetRXAGrphEQ(int channel, int *rxeq);                                       /* wdsp/eq.c:322-346 */
void SetRXAGrphEQ10(int channel, int *rxeq);                                     /* wdsp/eq.c:348-377 */
void SetRXAAMSQThreshold(int channel, double threshold);                         /* wdsp/amsq.c:224-232, dB */
void SetRXAAMSQMaxTail(int channel, double tail);                                /* wdsp/amsq.c:234-243, seconds */
void SetRXAEMNRRun(int channel, int run);                                        /* wdsp/emnr.c:1096-1110; needs the files `calculus` and
                                                                                    `zetaHat.bin` in the working directory or in $QH_WDSP_DATA, as WDSP reads them (emnr.c:212,317) */
void SetRXAEMNRnpeMethod(int channel, int method);                               /* wdsp/emnr.c:1120 */
void SetRXAEMNRaeRun(int channel, int run);                                      /* wdsp/emnr.c:1128 */
void SetRXAEMNRPosition(int channel, int position);                              /* wdsp/emnr.c:1136 */
void SetRXAEMNRaeZetaThresh(int channel, double v);
void SetRXAEMNRaePsi(int channel, double v);
void SetRXAEMNRtrainZetaThresh(int channel, double v);
void SetRXAEMNRtrainT2(int channel, double v);

void SetRXAEMNRgainMethod(int channel, int method);                              /* wdsp/emnr.c:1112: gain methods 0..3 */
void SetRXASNBARun(int channel, int run);                                        /* wdsp/snb.c:579-593 */
void SetRXASNBAOutputBandwidth(int channel, double flow, double fhigh);          /* wdsp/snb.c:660-694 */
void SetRXASNBAasize(int channel, int size);                                     /* wdsp/snb.c:604-658 */
void SetRXASNBAnpasses(int channel, int npasses);
void SetRXASNBAk1(int channel, double k1);
void SetRXASNBAk2(int channel, double k2);
void SetRXASNBAbridge(int channel, int bridge);
void SetRXASNBApresamps(int channel, int presamps);
void SetRXASNBApostsamps(int channel, int postsamps);
void SetRXASNBApmultmin(int channel, double pmultmin);
void SetRXASNBAovrlp(int channel, int ovrlp);

/* Status of the drop-in layer: 0 when the last WDSP-named call succeeded, else a qh_status. */
int qh_wdsp_status(void);
long long qh_wdsp_graph_launches(void);     /* DSP blocks replayed from a captured hipGraph (steady state of fexchange0) */

/* ------------------------------------------------------------------ 3. batched FIR decimator bank */
/* GPU form of quisk_cDecimate / quisk_cCDecimate / quisk_cFilter (filter.c:203-257,372-375; filter.h:47-55)
 * over `nch` independent complex streams that share one filter:
 *     y[m] = sum_k h[k] * x[decim*m + (decim-1-phase) - k],   phase = the reference's decim_index, kept
 * between calls like struct quisk_cFilter keeps it (filter.h:1-10), as is the ntaps-1 sample history.
 * taps_im == NULL: real taps (quisk_cDecimate); else complex taps as quisk_filt_tune() builds them
 * (quisk_cCDecimate).  With qh_hb45_taps() and decim 2 it is quisk_cDecim2HB45 (filter.c:377-417). */
typedef struct qh_fir qh_fir;
enum { QH_F64 = 0, QH_F32 = 1 };            /* sample type: interleaved complex double / complex float */

qh_fir *qh_fir_create(int device, int nch, const double *taps_re, const double *taps_im, int ntaps, int decim,
                      int dtype, void *stream);
void qh_fir_destroy(qh_fir *f);
int qh_fir_reset(qh_fir *f);                                   /* history and phase back to zero */
/* Load state from the host: hist = the ntaps-1 most recent samples per channel, oldest first ([nch][ntaps-1],
 * NULL = zeros); phase = decim_index (0 .. decim-1). */
int qh_fir_set_state(qh_fir *f, const void *hist, int phase);
int qh_fir_out_count(const qh_fir *f, int n_in);               /* outputs the next call with n_in samples produces */
/* d_in [nch][in_stride], d_out [nch][out_stride] device pointers (strides in complex samples); *n_out = outputs
 * per channel (may be 0).  Asynchronous on the filter's stream.  Output rows that share any byte with the input rows are refused
 * (QH_ERR_INVALID, nothing enqueued, no state moved); the _host form stages through device rows of its own and takes h_out == h_in. */
int qh_fir_process(qh_fir *f, const void *d_in, long long in_stride, int n_in, void *d_out, long long out_stride, int *n_out);
int qh_fir_process_host(qh_fir *f, const void *h_in, long long in_stride, int n_in, void *h_out, long long out_stride, int *n_out);
int qh_fir_synchronize(qh_fir *f);
/* The 43 taps (delays 0..42) of Quisk's 45-tap half-band whose outer taps are zero (filter.c:382-385). */
void qh_hb45_taps(double *taps43);

/* ------------------------------------------------------------------ 3b. fused half-band cascade */
/* `nstage` (1..8) consecutive quisk_cDecim2HB45 stages (filter.c:377-417; chained at quisk.c:1772-1796) over
 * `nch` complex streams in ONE pass over HBM: decimation 2^nstage, state (the input history) carried between
 * calls.  n_in must be a multiple of 2^nstage; n_in / 2^nstage outputs per channel.  dtype QH_F64 / QH_F32.
 * Results equal nstage calls of quisk_cDecim2HB45 to rounding (time-domain sums, not FFT).  Output rows that share any byte with the
 * input rows are refused (QH_ERR_INVALID, before anything runs): the time segments of a call run side by side (the drop-in
 * quisk_cDecim2HB45, which works in place like the reference's, goes through rows of its own; so does qh_hbc_process_host, h_out == h_in). */
typedef struct qh_hbc qh_hbc;
qh_hbc *qh_hbc_create(int device, int nch, int nstage, int dtype, void *stream);
void qh_hbc_destroy(qh_hbc *h);
int qh_hbc_reset(qh_hbc *h);
int qh_hbc_process(qh_hbc *h, const void *d_in, long long in_stride, int n_in, void *d_out, long long out_stride);
int qh_hbc_process_host(qh_hbc *h, const void *h_in, long long in_stride, int n_in, void *h_out, long long out_stride);
int qh_hbc_synchronize(qh_hbc *h);

/* ------------------------------------------------------------------ 3c. polyphase rational resampler */
/* quisk_cInterpDecim (filter.c:287-324) for `nch` complex streams, real taps; decim = 1 is quisk_cInterpolate
 * (filter.c:131-165); two real streams ride as the real and imaginary parts (quisk_dInterpolate, filter.c:167-201).
 * Output m sits at upsampled position p = phase + m*decim:  y[m] = interp * sum_k taps[p % interp + k*interp] *
 * x[p / interp - k].  `phase` (the reference's decim_index) and the last ceil(ntaps/interp)-1 inputs carry over. */
typedef struct qh_rat qh_rat;
qh_rat *qh_rat_create(int device, int nch, const double *taps, int ntaps, int interp, int decim, int dtype, void *stream);
void qh_rat_destroy(qh_rat *h);
int qh_rat_reset(qh_rat *h);
/* hist: [nch][ceil(ntaps/interp) - 1] complex samples of the stream's dtype, oldest first (NULL = zeros). */
int qh_rat_set_state(qh_rat *h, const void *hist, int phase);
int qh_rat_phase(const qh_rat *h);
int qh_rat_out_count(const qh_rat *h, int n_in);
/* Output rows that share any byte with the input rows are refused (QH_ERR_INVALID, state untouched); _host takes h_out == h_in. */
int qh_rat_process(qh_rat *h, const void *d_in, long long in_stride, int n_in, void *d_out, long long out_stride, int *n_out);
int qh_rat_process_host(qh_rat *h, const void *h_in, long long in_stride, int n_in, void *h_out, long long out_stride, int *n_out);
int qh_rat_synchronize(qh_rat *h);

/* ------------------------------------------------------------------ 5. batched panadapter */
/* Quisk's spectrum display path for `nch` receivers: the FFT ring producer of quisk_process_samples
 * (quisk.c:2454-2475), record_app's Hanning window (quisk.c:6003-6009) and get_graph job 1
 * (quisk.c:5142-5331: window, complex FFT, RMS S-meter over the passband bins, fftshift, |X| average,
 * box sum per pixel, 20*log10 - 20*(log10 count + log10 N + 31 log10 2), clamp [-200, 0]).
 * Every completed block of fft_size samples is transformed (the reference drops blocks when the GUI is
 * slow).  fft_size: any even size 16 .. 16384 ("FFT size must be an even number", quisk.py:186).  Powers of two from 1024 run
 * the fused kernel; the sizes Quisk itself picks (data_width * fft_mult with data_width = 2^a * y * z, quisk.py:186-194,4179:
 * 4000, 9600 ...) run Bluestein's algorithm on the power-of-two transforms, about three times the work. */
typedef struct qh_pan qh_pan;
qh_pan *qh_pan_create(int device, int nch, int fft_size, int data_width, double sample_rate, void *stream);
void qh_pan_destroy(qh_pan *p);
/* S-meter passband of channel ch (-1 = all): starts at f_start = rx_tune_freq + filter_start_offset (Hz, signed),
 * width = filter_bandwidth (quisk.c:5223-5229). */
int qh_pan_set_smeter_band(qh_pan *p, int ch, double f_start, double bandwidth);
/* Append n raw (pre-tune) IQ samples per channel, device pointer [nch][in_stride] complex double. */
int qh_pan_feed(qh_pan *p, const double *d_in, long long in_stride, int n);
int qh_pan_feed_host(qh_pan *p, const double *h_in, long long in_stride, int n);
int qh_pan_count(const qh_pan *p);          /* FFTs averaged since the last qh_pan_graph */
/* A decimating FIR on the panadapter's read: quisk_process_samples feeds the same cSamples to the FFT ring (quisk.c:2454-2475)
 * and to quisk_cDecimate (filter.c:203-229); with fft_size 16384, decimation 32 and up to 1024 real taps (BASELINE config 3) the
 * panadapter's own transform serves both (panfir16k_kernel, qh_pan.hip) and the stream is read once.  qh_pan_feed_decimate
 * takes whole blocks (n a multiple of fft_size, the panadapter at a block boundary) and writes n / decim samples per channel
 * exactly as quisk_cDecimate(cSamples, n, filter, decim) leaves them, state carried between calls; other shapes are refused
 * (QH_ERR_UNSUPPORTED): qh_fir beside qh_pan_feed does those.  Output rows that share any byte with the input rows are refused
 * (QH_ERR_INVALID, before the block count or the delay line moves). */
int qh_pan_attach_fir(qh_pan *p, const double *taps, int ntaps, int decim);
int qh_pan_feed_decimate(qh_pan *p, const double *d_in, long long in_stride, int n, double *d_out, long long out_stride, int *n_out);
/* The refresh branch of get_graph: h_pixels [nch][data_width] dB, h_smeter [nch] dB (either may be NULL),
 * *count = FFTs that were averaged (0: nothing was written, like get_graph returning None). */
int qh_pan_graph(qh_pan *p, double zoom, double deltaf, double *h_pixels, double *h_smeter, int *count);
/* The waterfall row of the same refresh: get_graph followed by watfall_OnGraphData
 * (quisk.c:5372-5421) -- colour index (int)((dB - gain + 40 + 0.69 y_zero) * (y_scale + 10) * 0.10 + 128) clamped to
 * 0..255 through the 256-entry red / green / blue tables of watfall_RgbData (quisk.c:5334); h_rgb [nch][width][3]
 * bytes, pixels past data_width black.  Resets the average like qh_pan_graph. */
int qh_pan_waterfall(qh_pan *p, double zoom, double deltaf, const unsigned char *red, const unsigned char *green,
                     const unsigned char *blue, int y_zero, int y_scale, double gain, int width, unsigned char *h_rgb,
                     double *h_smeter, int *count);
/* watfall_OnGraphData alone for `nrows` dB rows on the host: h_db [nrows][ncols] -> h_rgb [nrows][width][3]. */
int qh_watfall_rows_host(int device, const double *h_db, int nrows, int ncols, const unsigned char *red,
                         const unsigned char *green, const unsigned char *blue, int y_zero, int y_scale, double gain,
                         int width, unsigned char *h_rgb);

/* The bandscope (get_bandscope, quisk.c:4957-5011; 8(f) rank 4) for `nch` ADC streams: blocks of bandscope_size REAL
 * samples (already divided by bandscopeScale, quisk.c:3596) -> Hanning (init_bandscope, quisk.c:2887) -> r2c ->
 * |X[0 .. size/2]| averaged over the blocks; qh_bscope_graph is the refresh branch: copy2pixels (quisk.c:4932-4955:
 * fractional-bin box sums for the view (zoom, deltaf) of 0 .. clock / 2), scale, dB with floor -200, and
 * hermes_adc_level = the largest |sample| since the last call.  bandscope_size 1024 .. 16384, a power of two. */
typedef struct qh_bscope qh_bscope;
qh_bscope *qh_bscope_create(int device, int nch, int bandscope_size, int graph_width, void *stream);
void qh_bscope_destroy(qh_bscope *b);
int qh_bscope_feed(qh_bscope *b, const double *d_in, long long in_stride, int n);         /* [nch][in_stride] doubles */
int qh_bscope_feed_host(qh_bscope *b, const double *h_in, long long in_stride, int n);
int qh_bscope_count(const qh_bscope *b);
int qh_bscope_graph(qh_bscope *b, int clock, double zoom, double deltaf, double *h_pixels, double *h_adc_level, int *count);

/* ------------------------------------------------------------------ 6. Quisk-native receiver bank */
/* The receive path of quisk_process_samples (quisk.c:2289-2742) for `nch` receivers that share the sample rate
 * and the mode: NCO tune (quisk.c:2477-2488) -> quisk_process_decimate (quisk.c:1673-1846, PlanDecimation rates:
 * 48000 * 2^a 3^b 5^c) -> quisk_process_demodulate (quisk.c:1848-2068: CWL 0, CWU 1, LSB 2, USB 3, AM 4, FM 5, the
 * rx_mode_type values of quisk.h:55-70) with the Rx filter of set_filters -> mono to both channels.  Output: 48 ksps
 * complex (d + I*d).  process_agc, squelch, auto-notch and the noise blanker are not applied.
 * The seven coefficient tables are those of filters.h (98, 147, 245, 50, 36, 186, 309 values). */
typedef struct qh_qrx qh_qrx;
qh_qrx *qh_qrx_create(int device, int nch, int sample_rate, int mode, const double *quiskFilt48dec24Coefs,
                      const double *quiskFilt144D3Coefs, const double *quiskFilt240D5CoefsSharp,
                      const double *quiskAudio24p4Coefs, const double *quiskAudio24p6Coefs,
                      const double *quiskLpFilt48Coefs, const double *quiskAudioFmHpCoefs, void *stream);
void qh_qrx_destroy(qh_qrx *r);
int qh_qrx_filter_rate(const qh_qrx *r);                                   /* get_filter_rate, quisk.c:2787-2859 */
int qh_qrx_set_tune(qh_qrx *r, int ch, int rx_tune_freq);                   /* set_tune, quisk.c:4702; ch -1 = all */
int qh_qrx_set_tune_all(qh_qrx *r, const int *rx_tune_freq);                /* rx_tune_freq[nch]: every receiver's set_tune in ONE launch per table (bit-identical to nch calls) */
int qh_qrx_set_filters(qh_qrx *r, int ch, const double *filtI, const double *filtQ, int size);  /* set_filters, quisk.c:4551 */
int qh_qrx_out_count(const qh_qrx *r, int n_in);                            /* 48 ksps samples the next call returns */
/* Every rate and mode of the path: the filters.h tables by name (the last six may be NULL when the sample rate
 * does not need them: quiskFilt300D5Coefs for rates that land on 50-60 ksps and take the 6/5 x 4/5 stage,
 * quisk.c:1834-1838; the SDR-IQ tables for 53/111/133/185/370/740/1333 ksps, quisk.c:1732-1768).  `bandwidth` is
 * set_filters' third argument (quisk.c:4581): DGT-U/L and FDV-U/L filter at decim_rate/8 below 3000 Hz and at
 * decim_rate otherwise (quisk.c:2089), DGT-IQ is unfiltered from 19000 Hz up (quisk.c:2143).  Modes: rx_mode_type
 * (quisk.h:55-70) 0..13 except EXT (6, a user plugin); IMD takes the SSB path as in the reference; FDV-U/L stop at
 * the audio that the reference hands to the codec.  Output rate = qh_qrx_decim_rate() (48000 except SDR-IQ rates);
 * DGT-IQ output is the filtered IQ stream, every other mode (d, d). */
typedef struct qh_qrx_tables {
    const double *f48dec24, *f144d3, *f240d5, *audio24p4, *audio24p6, *lp48, *fmhp;         /* 98 147 245 50 36 186 309 */
    const double *f300d5, *sdriq53, *sdriq111, *sdriq133, *sdriq167, *sdriq185;             /* 125 55 114 136 174 189 */
} qh_qrx_tables;
qh_qrx *qh_qrx_create_ex(int device, int nch, int sample_rate, int mode, int bandwidth, const qh_qrx_tables *tables, void *stream);
int qh_qrx_decim_rate(const qh_qrx *r);
/* d_in [nch][in_stride] complex double at sample_rate, d_out [nch][out_stride] at 48 ksps; any n_in.  Output rows that share any byte
 * with the input rows are refused (QH_ERR_INVALID, state untouched); the _host form takes h_out == h_in. */
int qh_qrx_process(qh_qrx *r, const double *d_in, long long in_stride, int n_in, double *d_out, long long out_stride, int *n_out);
int qh_qrx_process_host(qh_qrx *r, const double *h_in, long long in_stride, int n_in, double *h_out, long long out_stride, int *n_out);
int qh_qrx_synchronize(qh_qrx *r);

/* ------------------------------------------------------------------ 7. wire-format sample ingest */
/* Quisk's sample sources left-justify 1-4 byte integer IQ in an int32 (full scale +-2^31) and, for UDP sources,
 * scale by rx_udp_gain_correct: quisk_read_rx_udp (quisk.c:3378-3392), add_rx_samples (quisk.c:2923-2952), the
 * Hermes / HPSDR frames of read_rx_udp10 (quisk.c:3745-3760).  This describes such a byte stream so that the GPU
 * reads it as it arrived: sample g of channel c starts at
 *   c*chan_stride + first_offset + (g / records_per_frame)*frame_stride + (g % records_per_frame)*record_stride
 * (records_per_frame 0 = one endless frame) and is two parts of sample_bytes bytes each.  Results are bit-exact
 * with the reference's conversion (integer -> double -> one multiply). */
typedef struct qh_iq_format {
    int sample_bytes;               /* 1..4 bytes per part */
    int big_endian;                 /* byte order of a part */
    int q_first;                    /* 1: the first part is the imaginary one (Hermes, quisk.c:3748-3750) */
    int records_per_frame;
    long long first_offset, record_stride, frame_stride;
    double gain;                    /* applied to the left-justified int32 (rx_udp_gain_correct; 1/2^31 for WDSP scale) */
} qh_iq_format;
void qh_iq_format_le24(qh_iq_format *f, double gain);               /* quisk_read_rx_udp, quisk.c:3378-3392 */
void qh_iq_format_hermes(qh_iq_format *f, int nrx, double gain);    /* read_rx_udp10 frames, quisk.c:3745-3760; channel r: chan_stride 6 */
/* d_src: packed bytes on the device; d_dst [nch][dst_stride] complex of `dtype`.  Output rows that share any byte with the
 * src_bytes of d_src are refused (QH_ERR_INVALID). */
int qh_unpack_iq(int device, void *stream, const void *d_src, long long src_bytes, const qh_iq_format *fmt, int nch,
                 long long chan_stride, int n, void *d_dst, long long dst_stride, int dtype);
/* qh_rxa_process with the decode fused into the first kernel's load: 6 bytes per sample cross HBM instead of 16
 * and no complex-double copy of the input exists.  nblk blocks of dsp_insize samples per channel.  Output rows that share any byte
 * with the src_bytes of d_src are refused (QH_ERR_INVALID, state untouched). */
int qh_rxa_process_packed(qh_rxa *e, const void *d_src, long long src_bytes, const qh_iq_format *fmt, long long chan_stride,
                          double *d_out, long long out_stride, int nblk);
/* The same two from host memory (upload, run, download, synchronize). */
int qh_unpack_iq_host(int device, const void *h_src, long long src_bytes, const qh_iq_format *fmt, int nch, long long chan_stride,
                      int n, void *h_dst, long long dst_stride, int dtype);
int qh_rxa_process_packed_host(qh_rxa *e, const void *h_src, long long src_bytes, const qh_iq_format *fmt, long long chan_stride,
                               double *h_out, long long out_stride, int nblk);

/* read_rx_udp17 (quisk.c:3821-3999), the two-stream UDP source: packets of 2 header bytes (sequence number; status, bit 1 =
 * ADC overrange) + 6-byte records, 24-bit little-endian I then Q left-justified in an int32 and scaled by rx_udp_gain_correct.
 * The LSB of I sorts every sample into the receiver's stream (clear: d_ch0, what the function returns in cSamples0) or the
 * panadapter's (set: d_ch1, conjugated when the spectrum is inverted, the DC estimate (dc_re, dc_im) removed); on the
 * panadapter stream a clear LSB of Q marks the first sample of a scan's first block (d_marks: slots of d_ch1).  The flag bits
 * stay in the sample values, as in the reference.  d_counts[4] = samples on channel 0, on channel 1, marks, packets with
 * the overrange bit; d_dc_sum[2] = sum of the channel-1 samples ahead of the DC removal: the caller keeps the estimate (the
 * reference renews it from that sum once a second of wall time, quisk.c:3947-3952).  Buffers: npackets * (packet_bytes - 2) / 6
 * entries each.  Bit-exact with the reference's loop.  Any byte shared by two of the six buffers (the source and each output) is
 * refused (QH_ERR_INVALID). */
int qh_unpack_udp17(int device, void *stream, const void *d_src, int npackets, int packet_bytes, double gain, int invert_spectrum,
                    double dc_re, double dc_im, void *d_ch0, void *d_ch1, int *d_marks, long long *d_counts, double *d_dc_sum);
int qh_unpack_udp17_host(int device, const void *h_src, int npackets, int packet_bytes, double gain, int invert_spectrum, double dc_re,
                         double dc_im, void *h_ch0, void *h_ch1, int *h_marks, long long *h_counts, double *h_dc_sum);

/* ------------------------------------------------------------------ 7b. audio egress */
/* The narrowing Quisk's sound back ends apply to the complex doubles a receive chain returns, done in the store of the
 * chain's last kernel so that 4 (Int16 stereo) instead of 16 bytes per output sample cross HBM:
 *   QH_AUDIO_I16   (short)(int)(volume * x / 65536)            sound_alsa.c:344-348, sound_pulseaudio.c:694-695
 *   QH_AUDIO_I24   three low bytes (LE) of (int)(volume * x / 256)                       sound_alsa.c:360-375
 *   QH_AUDIO_I32   (int)(volume * x)                           sound_alsa.c:386-390
 *   QH_AUDIO_F32   (float)(volume * x / CLIP32)                sound_pulseaudio.c:684-685, sound_portaudio.c:120-123
 * x = real / imaginary part at Quisk's +-2^31 scale.  prescale multiplies first (0 or 1: none): WDSP-scale chains (+-1.0)
 * pass 2147483647.0, the factor of quisk_wdsp.c:67.  A frame has num_channels slots; the real part goes to slot channel_I,
 * the imaginary part to slot channel_Q (struct sound_dev, quisk.h).  (int) truncates toward zero; it saturates where C
 * leaves the conversion undefined.  Bit-exact with the reference's expression for every in-range value. */
enum { QH_AUDIO_I16 = 1, QH_AUDIO_I24 = 2, QH_AUDIO_I32 = 3, QH_AUDIO_F32 = 4 };
typedef struct qh_audio_format {
    int kind, num_channels, channel_I, channel_Q;
    double volume, prescale;
} qh_audio_format;
/* qh_rxa_process with audio frames as output: d_out [nch][out_stride_bytes], nblk * dsp_outsize frames per channel.  Output rows
 * that share any byte with the input rows are refused (QH_ERR_INVALID, state untouched). */
int qh_rxa_process_audio(qh_rxa *e, const double *d_in, long long in_stride, void *d_out, long long out_stride_bytes, int nblk,
                         const qh_audio_format *fmt);
/* Stand-alone: d_src [nch][src_stride] complex double on the device -> frames.  Frames that share any byte with the source rows
 * are refused (QH_ERR_INVALID). */
int qh_audio_pack(int device, void *stream, const double *d_src, long long src_stride, int nch, int n, const qh_audio_format *fmt,
                  void *d_dst, long long dst_stride_bytes);

/* ------------------------------------------------------------------ 8. Quisk's audio AGC */
/* process_agc (quisk.c:2162-2287) for `nch` streams of complex double at `sample_rate` (the playback rate):
 * 15 ms look-ahead FIFO, gain ramp on overload, exponential release towards min(release gain, headroom).
 * max_out 0.7 and release_time 1.0 s are Quisk's values (quisk.c:2321,192); is_cpx selects |z| (EXT, DGT-IQ) or
 * |Re z| (every other mode, quisk.c:2686-2702).  As in the reference, the FIRST call only sets the state up and
 * leaves its samples untouched (quisk.c:2173-2190).  In place. */
typedef struct qh_qagc qh_qagc;
qh_qagc *qh_qagc_create(int device, int nch, int sample_rate, double max_out, double release_time, int is_cpx, void *stream);
void qh_qagc_destroy(qh_qagc *a);
int qh_qagc_set_gain(qh_qagc *a, int ch, double release_gain);          /* set_agc(d), quisk.c:4543; default 80 */
int qh_qagc_set_cpx(qh_qagc *a, int is_cpx);                            /* process_agc's is_cpx argument for the calls to come */
int qh_qagc_reset(qh_qagc *a);
int qh_qagc_process(qh_qagc *a, void *d_buf, long long stride, int n);
/* the same from one device buffer into another: d_src == d_dst with src_stride == dst_stride is qh_qagc_process (in place); any
 * other overlap of the two sets of rows is refused (QH_ERR_INVALID, AGC state untouched) */
int qh_qagc_process2(qh_qagc *a, const void *d_src, long long src_stride, void *d_dst, long long dst_stride, int n);
/* diagnostics: 0 = the two regimes of the state machine as instruction chains (default), 1 = the whole machine sample by sample
   (bit-identical, ~9 times slower) */
int qh_qagc_debug_form(qh_qagc *a, int form);
int qh_qagc_process_host(qh_qagc *a, void *h_buf, long long stride, int n);
/* The receiver bank with process_agc on its output, as quisk_process_samples has it; off by default. */
int qh_qrx_set_agc(qh_qrx *r, int on, double release_gain);
/* FM / DGT-FM banks: set_squelch(d) (quisk.c:4721); the block is zeroed while the mean |cx| (dB re full scale, over >= 2400
 * samples, evaluated per call: quisk.c:2076-2085) is below `level`.  Default -999: never. */
int qh_qrx_set_squelch(qh_qrx *r, int ch, double level);
/* one quisk_process_samples call handed over in pieces: 1 ahead of the first piece, 0 behind the last (the FM squelch's level is looked at once
 * per call, quisk.c:2076-2085, whether a threshold is set or not) */
int qh_qrx_squelch_pieces(qh_qrx *r, int pieces);
/* CW / SSB / AM banks: set_ssb_squelch(enabled, level) (quisk.c:4729): spectral-flatness squelch on 512-sample blocks of the
 * audio at the filter rate (ssb_squelch, quisk.c:1086-1180) plus the 512-sample audio delay that goes with it (d_delay). */
int qh_qrx_set_ssb_squelch(qh_qrx *r, int enabled, int level);

/* ------------------------------------------------------------------ 10. Quisk's noise blanker */
/* NoiseBlanker (quisk.c:680-784) for `nch` fp64 complex streams at the receiver's INPUT rate,
 * where quisk_process_samples runs it (quisk.c:2448-2449: before the panadapter ring and the tune).  While on, the
 * output lags the input by qh_nb_delay() = 3 * (int)(sample_rate * 500e-6 + 0.5) samples (the reference's delay
 * line); level 0 passes samples through undelayed and freezes the delay line, as the reference does.  Levels 1..3 =
 * threshold 6.0 / 4.0 / 2.5 times the mean magnitude (set_noise_blanker, quisk.c:4605).  Output rows that share any byte
 * with the input rows are refused (QH_ERR_INVALID, delay line untouched); the _host form takes h_out == h_in.  Sample rates up to about 3.5 MHz (the 500 us window has to fit one LDS tile). */
typedef struct qh_nb qh_nb;
qh_nb *qh_nb_create(int device, int nch, int sample_rate, void *stream);
void qh_nb_destroy(qh_nb *b);
int qh_nb_delay(const qh_nb *b);
int qh_nb_set_level(qh_nb *b, int level);
int qh_nb_reset(qh_nb *b);
int qh_nb_process(qh_nb *b, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n);
int qh_nb_process_host(qh_nb *b, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n);
int qh_nb_synchronize(qh_nb *b);
/* ------------------------------------------------------------------ 10b. WDSP's noise blanker (ANB) */
/* xanb (wdsp/nob.c:107-187) for `nch` fp64 complex streams at the receiver's input rate, where WDSP's callers run it: in front of
 * fexchange0.  Every channel has its own settings and state, so channels with different delays run in one launch.  While a channel
 * runs, its output lags its input by qh_anb_delay() = trans_count + adv_count samples (initBlanker, nob.c:33-52: max(2, (int)(tau *
 * samplerate)) + (int)(advtime * samplerate)); with run = 0 samples pass undelayed and the delay line and every other piece of state
 * stand still (nob.c:185-186).  The detector's average is stepped in time tiles whose start values come from a scan (qh_anb.hip): a
 * trigger can differ from a sample-serial run only where |x| lies within eps / (1 - backmult) of avg * threshold; given the triggers
 * the output is the reference's bit for bit.  htime survives a restart and is not set on entry to the hang state, as in the reference
 * (the first quiet hang lasts hang_count samples longer than the later ones).
 * Refused with QH_ERR_INVALID, nothing changed: tau or advtime outside [0, 0.002] and a rate outside (0, 1536000] (the reference sizes
 * wave[] and the delay line for these and never checks, nob.c:29-31,80-82), a backtau that is not finite and positive, a threshold that
 * is not finite, a negative hangtime, a hangtime * samplerate of 2^30 samples or more (hang_count is an int).  Setters: ch = -1 means
 * every channel; they take effect at the next process call. */
typedef struct qh_anb qh_anb;
qh_anb *qh_anb_create(int device, int nch, double samplerate, double tau, double hangtime, double advtime, double backtau, double threshold,
                      void *stream);                                             /* create_anb + initBlanker, nob.c:33-87; run = 1 */
void qh_anb_destroy(qh_anb *b);                                                  /* nob.c:89-97 */
int qh_anb_delay(qh_anb *b, int ch);                                             /* trans_count + adv_count, nob.c:36-41 */
int qh_anb_set_run(qh_anb *b, int ch, int run);                                  /* nob.c:348-354: resets nothing */
int qh_anb_set_samplerate(qh_anb *b, int ch, double samplerate);                 /* nob.c:365-373: initBlanker, a full restart that zeroes the delay line */
int qh_anb_set_tau(qh_anb *b, int ch, double tau);                               /* nob.c:375-383: restart */
int qh_anb_set_hangtime(qh_anb *b, int ch, double hangtime);                     /* nob.c:385-393: restart */
int qh_anb_set_advtime(qh_anb *b, int ch, double advtime);                       /* nob.c:395-403: restart */
int qh_anb_set_backtau(qh_anb *b, int ch, double backtau);                       /* nob.c:405-413: restart */
int qh_anb_set_threshold(qh_anb *b, int ch, double threshold);                   /* nob.c:415-422: resets nothing */
int qh_anb_flush(qh_anb *b, int ch);                                             /* flush_anb, nob.c:99-105: restart */
/* xanb (nob.c:107-187) over n >= 0 samples of every channel: device rows [nch][stride] of interleaved complex doubles, strides in
 * complex samples, asynchronous on the bank's stream.  Output rows that share a byte with the input rows are refused (QH_ERR_INVALID,
 * state untouched); the _host form (synchronous, pageable memory) takes h_out == h_in. */
int qh_anb_process(qh_anb *b, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n);
int qh_anb_process_host(qh_anb *b, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n);
int qh_anb_synchronize(qh_anb *b);
/* ------------------------------------------------------------------ 10c. WDSP's second noise blanker (NOB, "NB2") */
/* xnob (wdsp/nobII.c:157-495) for `nch` fp64 complex streams at the receiver's input rate, in front of fexchange0 like ANB.  Every
 * channel has its own settings and state.  While a channel runs, its output lags its input by qh_nob_delay() = adv_slew + adv + 1 +
 * max_imp_seq + hang + hang_slew + 10 samples (flush_nob, nobII.c:143-145; the counts are (int)(time * samplerate), nobII.c:40-44, with
 * max_imp_seq_time 0.025 s and both slew times `slewtime`, as create_nobEXT fixes them); with run = 0 samples pass undelayed and every
 * piece of state stands still (nobII.c:492-493).  mode: 0 zeros, 1 hold the 10-tap sum of the clean samples before the blank, 2 the mean
 * of that and the sum of the clean samples after it, 3 the sum after it, 4 a line between the two (nobII.c:288-320).  The detector's
 * average is stepped in time tiles whose start values come from a scan (qh_nob.hip): an impulse flag can differ from a sample-serial run
 * only where |x| lies within eps / (1 - backmult) of avg * threshold; given the flags the output is the reference's bit for bit, the
 * mode-4 line (repeated addition) included, and so are the reference's reads ahead of its write position, which find what the ring held
 * dline_size = 50690 samples earlier (nobII.c:94-98, 225-235, 264-276).
 * Refused with QH_ERR_INVALID, nothing changed: a rate outside (0, 1536000] or below 40 (max_imp_seq would be 0 and a blank would never
 * end); slewtime, hangtime or advtime outside [0, 0.002] (the reference sizes awave[], hwave[] and the ring for these and never checks,
 * nobII.c:29-34, 94-102); any setting whose delay reaches dline_size (1.536 MHz with every time at 0.002: flush_nob would start the write
 * position beyond the ring, nobII.c:145, 177); a backtau that is not finite and positive; a threshold that is not finite; a mode outside
 * 0..4.  Two departures besides: the gather of the ten clean samples after a blank (nobII.c:262-278) stops after one turn of the ring
 * and takes zeros for the taps it has not found, where the reference's loop does not return (fewer than ten unflagged slots in the ring:
 * a threshold below 1 on a steady signal); and the ten clean samples before a blank come from the last 50752 samples, zeros beyond,
 * where bfbuff could still hold older ones.  Setters: ch = -1 means every channel; they take effect at the next process call.  Every
 * call of a running channel copies that channel's history (50752 samples and their flags, 0.8 MB read and as much written), however
 * small n is. */
typedef struct qh_nob qh_nob;
qh_nob *qh_nob_create(int device, int nch, double samplerate, int mode, double slewtime, double hangtime, double advtime, double backtau,
                      double threshold, void *stream);                           /* create_nob + init_nob, nobII.c:36-124; run = 1 */
void qh_nob_destroy(qh_nob *b);                                                  /* nobII.c:126-138 */
int qh_nob_delay(qh_nob *b, int ch);                                             /* in_idx - out_idx, nobII.c:143-145 */
int qh_nob_set_run(qh_nob *b, int ch, int run);                                  /* nobII.c:649-656: resets nothing */
int qh_nob_set_mode(qh_nob *b, int ch, int mode);                                /* nobII.c:658-665: resets nothing; shows at the next impulse set-up */
int qh_nob_set_samplerate(qh_nob *b, int ch, double samplerate);                 /* nobII.c:676-684: init_nob, a full restart that zeroes the ring */
int qh_nob_set_tau(qh_nob *b, int ch, double tau);                               /* nobII.c:686-695: both slew times; restart */
int qh_nob_set_hangtime(qh_nob *b, int ch, double hangtime);                     /* nobII.c:697-705: restart */
int qh_nob_set_advtime(qh_nob *b, int ch, double advtime);                       /* nobII.c:707-715: restart */
int qh_nob_set_backtau(qh_nob *b, int ch, double backtau);                       /* nobII.c:717-725: restart */
int qh_nob_set_threshold(qh_nob *b, int ch, double threshold);                   /* nobII.c:727-734: resets nothing */
int qh_nob_flush(qh_nob *b, int ch);                                             /* flush_nob, nobII.c:140-155 */
/* xnob (nobII.c:157-495) over n >= 0 samples of every channel: device rows [nch][stride] of interleaved complex doubles, strides in
 * complex samples, asynchronous on the bank's stream.  Output rows that share a byte with the input rows are refused (QH_ERR_INVALID,
 * state untouched); the _host form (synchronous, pageable memory) takes h_out == h_in. */
int qh_nob_process(qh_nob *b, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n);
int qh_nob_process_host(qh_nob *b, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n);
int qh_nob_synchronize(qh_nob *b);
/* ------------------------------------------------------------------ 10d. WDSP's variable-ratio resampler (VARSAMP) */
/* xvarsamp (wdsp/varsamp.c:124-179) for `nch` fp64 complex streams, where WDSP's callers run it: behind fexchange0, between the
 * receiver's audio and a sound device whose clock is not the radio's (rmatch.c is built on it).  Every call takes n input samples and a
 * ratio correction `var` per channel and produces about n * var * out_rate / in_rate samples: the count of every channel comes back
 * with the samples.  Every channel has its own design (rates, R, band edges, gain), varmode, run and state; channels with the same
 * design share one copy of the R-times oversampled prototype h (calc_varsamp, varsamp.c:29-68: rsize = (int)(140 * norm_rate /
 * min_rate) taps per output, ncoef = rsize * R + 1 coefficients).  fc = 0 selects 0.95 * 0.45 * min_rate and fc_low < 0 selects -fc
 * (varsamp.c:52-57).  varmode 1 slides 1 / (var * nom_ratio) linearly from the previous call's value to this call's over the n samples,
 * varmode 0 steps it (varsamp.c:133-138).
 * A call is two kernels.  The control recurrence (inv_cvar, h_offset and isamps, varsamp.c:148-160,170-172) does not read the samples:
 * one lane per channel walks it, statement for statement in IEEE doubles, and leaves for every output sample the input sample it is
 * made at and the h_offset in force, and the channel's count.  The counts and the offsets are therefore the reference's bit for bit.
 * The filter kernel then makes every output sample on its own: the rsize coefficients interpolated between neighbours of h (hshift,
 * varsamp.c:112-122) times the newest rsize inputs, summed in the reference's order in fp64 (products may be fused).  The last
 * rsize - 1 inputs of every channel are kept behind the call, so n may be smaller than rsize.  run = 0 copies the n samples and
 * reports n; inv_cvar still follows the call's var, as in the reference (varsamp.c:129-138 stand in front of `if (a->run)`).
 * n = 0 is accepted and produces nothing: with varmode 0 inv_cvar takes the call's value, with varmode 1 it keeps the previous one (the
 * reference divides by size there, and keeps old_inv_cvar whatever the quotient is); nothing else moves.
 * Refused with QH_ERR_INVALID, state untouched: rates <= 0; a rate ratio beyond 16 either way (rsize > 2240); R < 1; ncoef above
 * 4194304; a gain, fc or fc_low that is not finite; a var that is not finite or lies outside [0.5, 2] (the reference never checks, and
 * its loop does not end for var <= 0); an out_stride below qh_varsamp_max_out(b, n, var); output rows that share a byte with the input
 * rows.  Setters: ch = -1 means every channel; they take effect at the next process call.  Every channel holds 2240 samples of history
 * twice (70 KB), whatever its rsize.
 * Not provided: rmatch.c.  Its ring, its control loop and xrmatchIN / xrmatchOUT are host threading on top of this call. */
typedef struct qh_varsamp qh_varsamp;
qh_varsamp *qh_varsamp_create(int device, int nch, int in_rate, int out_rate, int R, double fc, double fc_low, double gain, double var,
                              int varmode, void *stream);                        /* create_varsamp + calc_varsamp, varsamp.c:29-96; run = 1 */
void qh_varsamp_destroy(qh_varsamp *b);                                          /* varsamp.c:98-102 */
int qh_varsamp_flush(qh_varsamp *b, int ch);                                     /* flush_varsamp, varsamp.c:104-110: keeps inv_cvar */
int qh_varsamp_set_run(qh_varsamp *b, int ch, int run);                          /* resets nothing (varsamp.c:139,176) */
int qh_varsamp_set_varmode(qh_varsamp *b, int ch, int varmode);                  /* resets nothing (varsamp.c:133) */
/* setInRate_varsamp and setOutRate_varsamp, varsamp.c:193-205: calc_varsamp, which designs h again, empties the history, zeroes
 * h_offset and isamps and sets inv_cvar to 1 / (var * nom_ratio) with the var of the last call */
int qh_varsamp_set_rates(qh_varsamp *b, int ch, int in_rate, int out_rate);
/* setBandwidth_varsamp, varsamp.c:217-226: calc_varsamp as above, but only for a channel whose fc_low or fc_high changes */
int qh_varsamp_set_bandwidth(qh_varsamp *b, int ch, double fc_low, double fc_high);
int qh_varsamp_rsize(qh_varsamp *b, int ch);                                     /* rsize, varsamp.c:58: the taps of one output sample */
int qh_varsamp_synchronize(qh_varsamp *b);
/* The largest count the next call of n samples with these var (host, [nch]) could report on any channel: a bound from every channel's
 * earlier and new 1 / (var * nom_ratio), not the count itself (that hangs on state in device memory).  Negative: a qh_status. */
long long qh_varsamp_max_out(qh_varsamp *b, int n, const double *var);
/* xvarsamp (varsamp.c:124-179) over n >= 0 input samples of every channel: device rows [nch][stride] of interleaved complex doubles,
 * strides in complex samples, out_stride >= qh_varsamp_max_out(b, n, var); var: host, [nch], read before the call returns; d_count:
 * device, int[nch], the samples written to every output row (may be null).  Nothing is written behind a row's count.  Asynchronous on
 * the bank's stream.  The _host form (synchronous, pageable memory; h_count host, int[nch]) takes h_out == h_in. */
int qh_varsamp_process(qh_varsamp *b, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n, const double *var,
                       int *d_count);
int qh_varsamp_process_host(qh_varsamp *b, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n,
                            const double *var, int *h_count);
/* ------------------------------------------------------------------ 10e. WDSP's diversity combiner (DIV) */
/* xdiv (wdsp/div.c:67-95) for `ngroups` groups of up to eight phase-coherent receivers, fp64 complex, where WDSP's callers run it:
 * behind the blankers, in front of fexchange0.  Every group has its own run, nr (1..8), output (0..nr) and eight rotate pairs.  run = 0:
 * the output is receiver 0.  output != nr: the output is receiver `output`.  output == nr: the output is the sum over i = 0 .. nr-1, in
 * that order, of (Irotate[i] + j Qrotate[i]) times receiver i -- what nulls an interferer with two antennas.  The sum is the
 * reference's bit for bit: it starts from +0.0, and every product, the difference or sum inside the bracket and the accumulation are
 * rounded on their own, nothing fused (all-zero inputs with a negative rotate give +0.0).  There is no fp32 form, as in the reference.
 * Nothing is kept from call to call.  A call is one kernel launch for all groups, copies included: nr reads and one write per sample.
 * Rows: receiver i of group g lies at d_in + (g * group_stride + i * rx_stride) complex doubles, the output of group g at d_out +
 * g * out_stride.  An output row may be exactly one of its own group's receiver rows: d_out == d_in + k * rx_stride with out_stride ==
 * group_stride, for some k < 8.  The result is then the reference's with out == in[k]: its memset zeroes that receiver's samples before
 * they are read, so the receiver contributes the running sum in place of its samples (S <- S + rotate[k] S, with the partial sum of
 * receivers 0 .. k-1); a group that copies receiver k writes nothing, one that copies another receiver overwrites row k.
 * Refused with QH_ERR_INVALID, nothing written and no setting changed: any other sharing of bytes between an output row and a receiver
 * row that the call reads (a group reads its first nr rows when it mixes, else the one row it copies); n < 0; a stride below n (so
 * output rows never share bytes with each other); a group with run != 0 and output > nr at the call (the reference would read a
 * receiver pointer nobody set); at the setters nr outside 1..8, output outside 0..8, qh_div_set_rotate's nr outside 0..8, a null array,
 * a value that is not finite (the reference writes past Irotate[8] or reads what it was not given).  n == 0 is accepted and does
 * nothing.  The setters are order-free, as in the reference: nr may come before or after output; g = -1 means every group; they take
 * effect at the next process call. */
typedef struct qh_div qh_div;
qh_div *qh_div_create(int device, int ngroups, int run, int nr, void *stream);   /* create_div, div.c:31-48: output 0, rotates 0 */
void qh_div_destroy(qh_div *b);                                                  /* div.c:50-60 */
int qh_div_set_run(qh_div *b, int g, int run);                                   /* div.c:137-144 */
int qh_div_set_nr(qh_div *b, int g, int nr);                                     /* div.c:157-164 */
int qh_div_set_output(qh_div *b, int g, int output);                             /* div.c:168-175 */
/* div.c:179-187: the first nr values of both arrays; this nr is the call's own, not the group's */
int qh_div_set_rotate(qh_div *b, int g, int nr, const double *Irotate, const double *Qrotate);
/* The settings of group g as the next call will use them; any pointer may be null; Irotate8 / Qrotate8: 8 doubles each */
int qh_div_get(qh_div *b, int g, int *run, int *nr, int *output, double *Irotate8, double *Qrotate8);
int qh_div_synchronize(qh_div *b);
/* xdiv (div.c:67-95) over n >= 0 samples of every group: device rows of interleaved complex doubles, strides in complex samples,
 * asynchronous on the bank's stream.  The _host form (synchronous, pageable memory) takes the same layouts, the in-place one included. */
int qh_div_process(qh_div *b, const void *d_in, long long rx_stride, long long group_stride, void *d_out, long long out_stride, int n);
int qh_div_process_host(qh_div *b, const void *h_in, long long rx_stride, long long group_stride, void *h_out, long long out_stride, int n);
/* dAutoNotch (quisk.c:786-963; 8(f) rank 3) inside the receiver bank, where the mode calls it (on the real audio after
 * the Rx filter; after the interpolators for FM; DGT-IQ has none): set_auto_notch(i) (quisk.c:4596) -- stores the flag
 * and starts the notch over -- with rit_freq as set_sidetone passes it (quisk.c:4712): the CW modes keep the notch off
 * the sidetone.  Off by default. */
int qh_qrx_set_auto_notch(qh_qrx *r, int on, int rit_freq);
/* The receiver bank with the blanker in front of its tune, as quisk_process_samples has it; 0 = off (default). */
int qh_qrx_set_noise_blanker(qh_qrx *r, int level);

/* ------------------------------------------------------------------ 10f. WDSP's fixed-ratio resampler (RESAMPLE, RESAMPLEF) */
/* xresample (wdsp/resample.c:121-157) for `nch` fp64 complex streams, or xresampleF (resample.c:296-330) for `nch` fp32 real streams
 * whose ring, taps and sums are fp64 ((double)in[i] on the way in, (float)I on the way out), as a stand-alone stream: a call takes n
 * input samples of every channel and reports how many output samples it made of each, so rate ratios that are whole in neither
 * direction (48 k -> 44.1 k) run as a proper stream.  Every channel has its own design, run and state; channels with equal designs
 * share one copy of the taps.  calc_resample (resample.c:35-78): L = out_rate / gcd, M = in_rate / gcd; fc = 0 selects 0.45 min_rate;
 * fc_low < 0 selects -fc; ncoef = 0 selects (int)(140 in_rate L / min_rate); ncoef is rounded up to (ncoef / L + 1) L, cpp = ncoef / L
 * taps meet every output.  The real-float form has create_resampleF's design instead (resample.c:250-273): fc = 0.45 min_rate, ncoef =
 * (int)(60 / fc_norm) rounded the same way, gain 1; the fc, ncoef and gain given to create are not used there.
 * Output m of a call sits at upsampled position p = phnum + m M: tap row p % L of the phase-major h[L][cpp] against inputs p / L,
 * p / L - 1, ..., summed j = 0 .. cpp - 1 in fp64 as resample.c:139-144 (products may be fused), with the last cpp - 1 inputs of the
 * earlier calls in front of the call's first sample.  The count, ceil((n L - phnum) / M), and the next phnum are evaluated on the host:
 * `counts` is filled when process returns, and no device count exists.  A call is one kernel, the history behind it included.
 * A new design (set_rates always; set_fc_low and set_bandwidth only when a value changes, resample.c:185-204) empties the channel's
 * history and sets its phase to 0, as calc_resample does.  n = 0 is accepted, makes nothing and moves nothing.
 * Deviations: run = 0 copies the channel's n samples and reports 0, what xresample returns (the V names fix run = 1).  Refused with
 * QH_ERR_INVALID, nothing changed: rates <= 0; in_rate * L beyond int (the reference's full_rate overflows); ncoef < 0; ncoef beyond
 * 4194304 after rounding; an fc, fc_low or gain that is not finite; set_fc_low and set_bandwidth on the real-float form; an out_stride
 * below qh_resample_max_out(b, n); output rows that share a byte with the input rows; a null handle or pointer.  The reference checks
 * none of these.  Setters: ch = -1 means every channel; they take effect at the next process call. */
enum { QH_RESAMPLE_C64 = 0, QH_RESAMPLE_R32 = 1 };  /* interleaved complex doubles / real floats */
typedef struct qh_resample qh_resample;
qh_resample *qh_resample_create(int device, int nch, int in_rate, int out_rate, double fc, int ncoef, double gain, int dtype,
                                void *stream);                                   /* create_resample, resample.c:86-103; create_resampleF, 236-280; run = 1 */
void qh_resample_destroy(qh_resample *b);                                        /* resample.c:105-110, 282-287 */
int qh_resample_set_run(qh_resample *b, int ch, int run);                        /* resets nothing (resample.c:124,154) */
int qh_resample_set_rates(qh_resample *b, int ch, int in_rate, int out_rate);    /* setInRate_ / setOutRate_resample, resample.c:171-183 */
int qh_resample_set_fc_low(qh_resample *b, int ch, double fc_low);               /* setFCLow_resample, resample.c:185-193 */
int qh_resample_set_bandwidth(qh_resample *b, int ch, double fc_low, double fc_high);    /* setBandwidth_resample, resample.c:195-204 */
int qh_resample_flush(qh_resample *b, int ch);                                   /* flush_resample, resample.c:112-118 (setSize_resample: 165-169) */
int qh_resample_L(qh_resample *b, int ch);                                       /* resample.c:53 */
int qh_resample_M(qh_resample *b, int ch);                                       /* resample.c:54 */
int qh_resample_cpp(qh_resample *b, int ch);                                     /* resample.c:66 */
/* the phase-major h[L][cpp] in force on channel ch (resample.c:69-72) -> out, which has room for cap doubles; returns L * cpp */
int qh_resample_taps(qh_resample *b, int ch, double *out, int cap);
/* what the next call of n samples makes of channel ch (0 while it does not run); negative: a qh_status */
long long qh_resample_out_count(qh_resample *b, int ch, int n);
/* the most samples a call of n samples can write to any output row, whatever the phases: ceil(n L / M) of a channel that runs, n of
 * one that does not; negative: a qh_status */
long long qh_resample_max_out(qh_resample *b, int n);
/* xresample / xresampleF over n >= 0 input samples of every channel: device rows [nch][stride] of the bank's sample type, strides in
 * samples, out_stride >= qh_resample_max_out(b, n); counts: host, int[nch], the samples made of every channel.  Nothing is written
 * behind a row's count (behind n for a channel that does not run).  Asynchronous on the bank's stream.  The _host form (synchronous,
 * pageable memory) takes h_out == h_in. */
int qh_resample_process(qh_resample *b, const void *d_in, long long in_stride, void *d_out, long long out_stride, int n, int *counts);
int qh_resample_process_host(qh_resample *b, const void *h_in, long long in_stride, void *h_out, long long out_stride, int n, int *counts);
int qh_resample_synchronize(qh_resample *b);
/* ------------------------------------------------------------------ 11. WDSP display engine (analyzer) */
/* wdsp/analyzer.c for a bank of `ndisp` displays that share one configuration: Spectrum0's sample
 * rings, the windowed transform every size - overlap samples, clip / flip / stitch (Celiminate, eliminate, stitch,
 * analyzer.c:179-279,555-600), the five detectors or the bin interpolation (detector, :282-461), the five averaging modes
 * (avenger, :463-553), the calibration spline (SetCalibration / build_interpolants / interpolate, :747-882,1380-1410) and
 * GetPixels (:1315).  The reference's dispatcher and worker threads become: every frame that is complete when a feed call
 * returns has been computed, in order.  fft sizes: powers of two from 512 to 8192 * 64; one LO per sub-span (dMAX_NUM_FFT = 1,
 * comm.h:125); SnapSpectrum is not built.  Samples are (I, Q) doubles; they are kept as floats like the reference's dINREAL
 * rings (comm.h:128-132).  Setters take the reference's arguments (analyzer.c:999-1017,1582-1676). */
typedef struct qh_ana qh_ana;
qh_ana *qh_ana_create(int device, int ndisp, int max_size, int max_stitch, void *stream);
void qh_ana_destroy(qh_ana *a);
int qh_ana_set_analyzer(qh_ana *a, int n_pixout, int n_fft, int typ, const int *flp, int sz, int bf_sz, int win_type, double pi, int ovrlp, int clp,
                        double fscLin, double fscHin, int n_pix, int n_stch, int calset, double fmin, double fmax, int max_w);
int qh_ana_set_calibration(qh_ana *a, int set_num, int n_points, const double *cal /* n_points rows of (frequency, value) */);
int qh_ana_set_detector_mode(qh_ana *a, int pixout, int mode);
int qh_ana_set_average_mode(qh_ana *a, int pixout, int mode);
int qh_ana_set_num_average(qh_ana *a, int pixout, int num);
int qh_ana_set_av_backmult(qh_ana *a, int pixout, double mult);
int qh_ana_set_sample_rate(qh_ana *a, int rate);
int qh_ana_set_norm_onehz(qh_ana *a, int pixout, int norm);
double qh_ana_get_enb(qh_ana *a);
int qh_ana_reset_pixel_buffers(qh_ana *a);
/* n = k * buff_size samples for sub-span ss of every display: d_iq[ndisp][disp_stride] on the device (qh_ana_feed) or in host
 * memory (qh_ana_feed_host; swap_iq = 1 reads Spectrum0's (Q, I) pair order).  *frames = pixel rows published by this call. */
int qh_ana_feed(qh_ana *a, int ss, const void *d_iq, long long disp_stride, int n, int *frames);
int qh_ana_feed_host(qh_ana *a, int ss, const double *h_iq, long long disp_stride, int n, int swap_iq, int *frames);
/* The same for (I, Q) float pairs on the device, as xsender leaves them; swap_iq = 1 reads Spectrum2's (Q, I) pair order.  The bank's
 * stream reads the rows behind everything producer_stream holds when the call is made (an event, no host wait); NULL: already ordered. */
int qh_ana_feed_f32(qh_ana *a, int ss, const void *d_iq, long long disp_stride, int n, int swap_iq, void *producer_stream, int *frames);   /* wdsp/sender.c:81 -> Spectrum2, analyzer.c:1490-1533 */
/* xsender -> Spectrum2 bank to bank, on the device: attach makes every later process call of the engine (device, host, packed, audio) end
 * by feeding its dsp_size * nblk sender samples per channel to sub-span ss, display d from channel d, in the pair order Spectrum2 reads
 * (swap_iq = 1: it takes element 2i + 1 as I, analyzer.c:1503-1507, of rows xsender hands over unswapped).  It needs ndisp = the engine's
 * channels, buff_size = dsp_size and the engine's device, switches every channel's sender on and refuses to switch one off while attached.
 * The two streams are ordered by events both ways.  a = NULL detaches (the senders stay on); the bank must outlive the attachment.
 * feed_display does one such feed of the last call's rows (every channel's sender on). */
int qh_rxa_attach_display(qh_rxa *e, qh_ana *a, int ss);                           /* wdsp/sender.c:81 */
int qh_rxa_feed_display(qh_rxa *e, qh_ana *a, int ss);                             /* wdsp/sender.c:81 */
/* GetPixels for one display of the bank: *flag = 1 and num_pixels floats (dB) if a row has been published since the last read */
int qh_ana_get_pixels(qh_ana *a, int disp, int pixout, float *pix, int *flag);
/* every row of the last feed call, [ndisp][frames][num_pixels] floats: device pointer / host copy */
int qh_ana_rows(qh_ana *a, int pixout, const float **d_rows, int *frames, int *num_pixels);
int qh_ana_rows_host(qh_ana *a, int pixout, float *out, int max_frames, int *frames);
/* SnapSpectrum (analyzer.c:1337-1367): the complex transform of the next frame of (display, sub-span), 2 * size doubles, fft-shifted
 * (bins size/2 .. size-1, then 0 .. size/2-1, analyzer.c:710-711).  arm, feed, take; or arm and wait while another thread feeds. */
int qh_ana_snap_arm(qh_ana *a, int disp, int ss);
int qh_ana_snap_take(qh_ana *a, double *snap_buff, int *flag);
int qh_ana_snap_wait(qh_ana *a, double *snap_buff, int timeout_ms, int *flag);
void *qh_ana_stream(qh_ana *a);
long long qh_ana_frames(qh_ana *a);
int qh_ana_buff_size(qh_ana *a);
int qh_ana_ndisp(qh_ana *a);
int qh_ana_device(qh_ana *a);
int qh_ana_num_stitch(qh_ana *a);
int qh_ana_num_pixels(qh_ana *a);
/* WDSP's own names and signatures (wdsp/analyzer.h:100-193, wdsp.h), one display per id 0..63, host pointers */
void XCreateAnalyzer(int disp, int *success, int m_size, int m_LO, int m_stitch, char *app_data_path);
void DestroyAnalyzer(int disp);
void SetAnalyzer(int disp, int n_pixout, int n_fft, int typ, int *flp, int sz, int bf_sz, int win_type, double pi, int ovrlp, int clp, double fscLin,
                 double fscHin, int n_pix, int n_stch, int calset, double fmin, double fmax, int max_w);
void SetCalibration(int disp, int set_num, int n_points, double (*cal)[2]);
void Spectrum0(int run, int disp, int ss, int LO, double *pbuff);
void Spectrum2(int run, int disp, int ss, int LO, float *pbuff);
void Spectrum(int disp, int ss, int LO, float *pI, float *pQ);
void OpenBuffer(int disp, int ss, int LO, void **Ipointer, void **Qpointer);
void CloseBuffer(int disp, int ss, int LO);
void GetPixels(int disp, int pixout, float *pix, int *flag);
void SnapSpectrum(int disp, int ss, int LO, double *snap_buff);
void SnapSpectrumTimeout(int disp, int ss, int LO, double *snap_buff, unsigned int timeout, int *flag);
void ResetPixelBuffers(int disp);
void SetDisplayDetectorMode(int disp, int pixout, int mode);
void SetDisplayAverageMode(int disp, int pixout, int mode);
void SetDisplayNumAverage(int disp, int pixout, int num);
void SetDisplayAvBackmult(int disp, int pixout, double mult);
void SetDisplaySampleRate(int disp, int rate);
void SetDisplayNormOneHz(int disp, int pixout, int norm);
double GetDisplayENB(int disp);

/* ------------------------------------------------------------------ 9. Quisk native block API, one receiver */
/* The shape of quisk.c's own receive API: a process-wide receiver, parameters through setters, samples through
 * `int quisk_process_samples(complex double *cSamples, int nSamples)` (quisk.h:375, quisk.c:2289) -- in place, returns
 * the output count at the playback rate, nSamples <= 0 returned unchanged.  process_agc is on as in the reference
 * (default release gain 80, quisk.c:191).  qh_quisk_open takes quisk_sound_state.sample_rate and .playback_rate (open_sound,
 * quisk.c:4106; 48000 x 1, 2, 4 or 8 -- the ratios quisk.c:2663-2682 interpolates), the filters.h tables and record_app's
 * fft_size / data_width (0, 0 = no panadapter).  The whole of quisk_process_samples (quisk.c:2289-2742) runs behind
 * qh_quisk_process_samples; the block is uploaded once and every step is a kernel on one stream (qh_quisk_rx_compat.cpp). */
int qh_quisk_open(int sample_rate, int playback_rate, const qh_qrx_tables *tables, int fft_size, int data_width);
void qh_quisk_close(void);
void qh_quisk_set_tune(int rx_tune_freq);                   /* set_tune, quisk.c:4702 */
void qh_quisk_set_rx_mode(int mode);                        /* set_rx_mode, quisk.c:4621 */
int qh_quisk_set_filters(const double *filtI, const double *filtQ, int size, int bandwidth);       /* set_filters, quisk.c:4551 */
void qh_quisk_set_agc(double level);                        /* set_agc, quisk.c:4543 */
void qh_quisk_set_noise_blanker(int level);                 /* set_noise_blanker, quisk.c:4605 */
void qh_quisk_set_auto_notch(int on, int rit_freq);         /* set_auto_notch, quisk.c:4596: the flag and the notch's restart.  rit_freq is IGNORED (kept for callers of earlier
                                                                 versions): the RIT is the one qh_quisk_set_sidetone set, the reference's global (quisk.c:4712) -- it also tunes the split
                                                                 receiver (quisk.c:2538) */
int qh_quisk_get_filter_rate(void);                         /* get_filter_rate(-1, 0), quisk.c:2787 */
int qh_quisk_process_samples(double *cSamples, int nSamples);       /* quisk_process_samples, quisk.c:2289.  In place, like the reference: cSamples is the caller's
                                                                         block buffer (SAMP_BUFFER_SIZE = 66000 samples in Quisk) and must hold the OUTPUT too -- up to (nSamples / decimation
                                                                         + one WDSP block when the shim is in use) x playback_rate / 48000 samples */
int qh_quisk_get_graph(double zoom, double deltaf, double *pixels, double *smeter);                /* get_graph, quisk.c:5142 */
/* get_filter (quisk.c:5481-5568): the Rx filter's response as the "RX Filter" screen draws it -- a multitone through the copy of the
 * cRxFilterOut loop that function carries, record_app's window, a data_width-point transform; db[data_width], negative frequencies
 * first, floor -140.  All sizeFilter taps of set_filters (up to MAX_FILTER_SIZE).  Returns data_width (0: error). */
int qh_quisk_get_filter(double *db);
/* The rest of quisk_process_samples' orchestration (quisk.c:2289-2742): a second receiver bank whose audio shares the
 * stereo output with the first -- split Rx/Tx (the same samples at tx_tune + rit, split modes 1..4 of quisk.c:2548-2590) or
 * the played sub-receiver (its own samples, frequency, mode and nFilter-1 filter; play methods 0..2 of quisk.c:2601-2620) --
 * with one AGC per output channel (Agc1 / Agc2, quisk.c:2690-2698); the key-down replacement of the block by sidetone or
 * silence, the TxRxSilenceMsec of silence after it and the 5 ms key-up ramp (quisk.c:2368-2433,2729-2738); kill_audio;
 * invert_spectrum. */
void qh_quisk_set_tx_tune(int tx_tune_freq);                               /* set_tune's second argument, quisk.c:4702 */
void qh_quisk_set_split_rxtx(int split);                                   /* set_split_rxtx, quisk.c:4694 */
void qh_quisk_set_multirx_play_channel(int ch);                            /* quisk.c:4856 */
void qh_quisk_set_multirx_play_method(int method);                         /* quisk.c:4846 */
void qh_quisk_set_multirx_freq(int index, int freq);                       /* quisk.c:4826 */
void qh_quisk_set_multirx_mode(int index, int mode);                       /* quisk.c:4836 */
int qh_quisk_multirx_samples(int index, const double *cSamples, int nSamples);     /* multirx_cSamples[index] for the next block */
int qh_quisk_set_filters2(const double *filtI, const double *filtQ, int size, int bandwidth);      /* set_filters(..., nFilter 1) */
void qh_quisk_set_key_state(int key_down, int cw_key_down, int active_sidetone, int is_fdx);
void qh_quisk_set_sidetone(double volume, int rit_freq, int playback_rate, int txrx_silence_msec);     /* set_sidetone, quisk.c:4710 */
void qh_quisk_set_kill_audio(int kill);
void qh_quisk_invert_spectrum(int invert);                                 /* quisk.c:4535 */
/* The tail and the side paths of quisk_process_samples: set_filters for any nFilter (0 main / split, 1 played sub-receiver,
 * 2 sub-receiver 1's digital output; one global sizeFilter as in quisk.c:4591); the squelches; add_tone (quisk.c:3203) and
 * AddTestTone (quisk.c:1258-1303); measure_frequency (quisk.c:3181) and measure_freq (quisk.c:5579-5649); sub-receiver 1
 * demodulated to a digital output device (quisk.c:2630-2651: quisk_multirx_count, the device's driver flag, the audio that
 * play_sound_interface is handed).  cFracDecim (quisk.c:622-665), the wdspFexchange0 hand-off (channel 0, when
 * qh_wdsp_set_parameter switched it on) and the HB45 interpolation to the playback rate need no setter. */
int qh_quisk_set_filters_n(const double *filtI, const double *filtQ, int size, int bandwidth, int nFilter);   /* set_filters, quisk.c:4551 */
void qh_quisk_set_squelch(double level);                                   /* set_squelch (FM), quisk.c:4721 */
void qh_quisk_set_ssb_squelch(int enabled, int level);                     /* set_ssb_squelch, quisk.c:4729 */
int qh_quisk_squelch_flags(void);                                          /* bit 0 squelch_real, bit 1 squelch_imag of the last block */
/* quisk_process_samples has no error return (failures are QuiskPrintf + counters, quisk.c:55): a call whose device chain failed returns
 * 0 samples, qh_last_error() says why, and this counter says that it happened (0 samples alone also means "no output yet") */
long long qh_quisk_error_count(void);
/* Mode EXT (quisk.c:2490-2493): the tuned block goes to the user's quisk_extern_demod (extdemod.c:13 -- `complex double *` in place,
 * returns the play-sample count <= nSamples) and from there straight to process_agc.  The reference links the function in; here it
 * is registered (a binding passes &quisk_extern_demod).  It is host code: the block makes one round trip.  Without one, mode EXT
 * fails loudly. */
void qh_quisk_set_extern_demod(int (*fn)(double *cSamples, int nSamples, double decim));
void qh_quisk_add_tone(int freq);                                          /* add_tone, quisk.c:3203 */
double qh_quisk_measure_frequency(int mode);                               /* measure_frequency, quisk.c:3181 */
void qh_quisk_set_multirx_count(int n);                                    /* quisk_multirx_count */
void qh_quisk_set_sub_rx1_output(int on);                                  /* quiskPlaybackDevices[QUISK_INDEX_SUB_RX1]->driver */
int qh_quisk_sub_rx1_audio(double *cSamples, int cap);                     /* the block play_sound_interface got, quisk.c:2651 */
/* ------------------------------------------------------------------ 9b. quisk_process_samples for a bank of receivers */
/* The whole of quisk_process_samples (quisk.c:2289-2742) for `nch` receivers side by side -- the batched form SURVEY.md 8(b) asks
 * for beside the drop-in symbols: AddTestTone / inversion (quisk.c:2438-2446), NoiseBlanker (:2448), the FFT ring feed on the same
 * samples (:2454-2475), tune + quisk_process_decimate + quisk_process_demodulate (:2477-2530), cFracDecim (:2654), the HB45
 * interpolation to the playback rate (:2663-2682), process_agc (:2686-2702, always on as in the reference) and kill_audio / the
 * squelches (:2712-2728).  Per receiver: tune frequency, Rx filter, FM squelch level; the rest are the bank's, as they are
 * process-wide globals in the reference.  The operator's side of the function (key-down replacement, key-up envelope, split and
 * sub-receiver channels, measure_freq, the WDSP hand-off) stays with the one-receiver API of group 9, which runs the same kernels
 * with nch = 1 (qh_ps_kernels.hpp).  fft_size / data_width 0, 0 = no panadapter.  stream NULL = a stream of the bank's own. */
typedef struct qh_qps qh_qps;
qh_qps *qh_qps_create(int device, int nch, int sample_rate, int playback_rate, int mode, int bandwidth, const qh_qrx_tables *tables,
                      int fft_size, int data_width, void *stream);
void qh_qps_destroy(qh_qps *h);
int qh_qps_set_tune(qh_qps *h, int ch, int rx_tune_freq);                  /* set_tune, quisk.c:4702; ch -1 = all */
int qh_qps_set_tune_all(qh_qps *h, const int *rx_tune_freq);               /* rx_tune_freq[nch], one launch per table for the whole bank */
int qh_qps_set_filters(qh_qps *h, int ch, const double *filtI, const double *filtQ, int size);     /* set_filters, quisk.c:4551 */
int qh_qps_set_agc(qh_qps *h, double level);                               /* set_agc, quisk.c:4543 (agcReleaseGain, default 80) */
int qh_qps_set_noise_blanker(qh_qps *h, int level);                        /* set_noise_blanker, quisk.c:4605 */
int qh_qps_set_auto_notch(qh_qps *h, int on, int rit_freq);                /* set_auto_notch, quisk.c:4596 */
int qh_qps_invert_spectrum(qh_qps *h, int invert);                         /* quisk.c:4535 */
int qh_qps_set_kill_audio(qh_qps *h, int kill);
int qh_qps_add_tone(qh_qps *h, int freq);                                  /* add_tone, quisk.c:3203; 0 = off */
int qh_qps_set_squelch(qh_qps *h, int ch, double level);                   /* set_squelch, quisk.c:4721: looked at by the FM demodulator alone -- accepted and without effect in a bank of another mode, like the reference's */
int qh_qps_set_ssb_squelch(qh_qps *h, int enabled, int level);             /* set_ssb_squelch, quisk.c:4729: CW, SSB and AM banks; accepted and without effect in an FM bank */
/* long calls run as `pieces` time pieces, process_agc of one beside the filters of the next (0 = chosen by call length) */
int qh_qps_set_pieces(qh_qps *h, int pieces);
int qh_qps_set_pipelined(qh_qps *h, int on);                               /* streaming callers: a call returns with its AGC still running and the next call's filters start beside it;
                                                                              output rows are complete after qh_qps_synchronize.  Same samples. */
int qh_qps_filter_rate(qh_qps *h);                                         /* get_filter_rate, quisk.c:2787 */
int qh_qps_decim_rate(qh_qps *h);
int qh_qps_out_capacity(qh_qps *h, int n_in);                              /* the most playback samples a call of n_in returns: out_stride >= this */
/* device rows [nch][stride] of complex doubles; *n_out = playback samples per receiver; asynchronous on the bank's stream.  Output rows
 * (qh_qps_out_capacity long) that share any byte with the input rows are refused (QH_ERR_INVALID, state untouched); _host takes h_out == h_in. */
int qh_qps_process(qh_qps *h, const double *d_in, long long in_stride, int n, double *d_out, long long out_stride, int *n_out);
int qh_qps_process_host(qh_qps *h, const double *h_in, long long in_stride, int n, double *h_out, long long out_stride, int *n_out);
int qh_qps_synchronize(qh_qps *h);
int qh_qps_squelch_flags(qh_qps *h, int *flags);                           /* squelch_real of every receiver after the last call */
int qh_qps_get_graph(qh_qps *h, double zoom, double deltaf, double *pixels, double *smeter, int *count);   /* get_graph, quisk.c:5142 */

/* Plumbing between the block API and the engines it chains (device-resident; used by qh_quisk_rx_compat.cpp): the bank
 * leaves the squelch to its caller and says where the flag lives; ssb_squelch's one-for-all-banks `plan` static
 * (quisk.c:1091,1104) and the one bandwidth it reads for all banks (filter_bandwidth[0], quisk.c:1120); the tuning oscillator's phase in 2^-64 turns (one vector per purpose in the reference,
 * quisk.c:2308-2311); measure_freq's window and averaged spectrum on the panadapter engine; the shim's state. */
int qh_qrx_set_mute_deferred(qh_qrx *r, int on);
const int *qh_qrx_squelch_flag(qh_qrx *r, int ch);
int qh_qrx_ssb_squelch_planned(qh_qrx *r, int set);
int qh_qrx_set_ssb_squelch_bandwidth(qh_qrx *r, int bandwidth);       /* filter_bandwidth[0]: what ssb_squelch reads in every bank (quisk.c:1120) */
int qh_qrx_get_nco_phase(qh_qrx *r, int ch, unsigned long long *phase);
int qh_qrx_set_nco_phase(qh_qrx *r, int ch, unsigned long long phase);
int qh_pan_set_window(qh_pan *p, const double *window);
int qh_pan_read_avg(qh_pan *p, double *h_avg, int reset);
int qh_pan_drop_partial(qh_pan *p);
int qh_wdsp_shim_in_size(int channel);

/* ------------------------------------------------------------------ 4. filter.h drop-in exports */
/* The reference's own names and struct layouts (filter.h:1-55) so that quisk.c links against this library
 * instead of filter.o.  `double *` stands for `complex double *` (same ABI: interleaved re, im).  Each call
 * takes the filter state from the caller's struct (circular history, ptcSamp, decim_index / toggle), runs the
 * block on the GPU and writes the state back in the reference's format, so calls may be mixed freely with the
 * reference's own functions on the same struct.  Errors (no device ...) return 0 samples and set
 * qh_last_error(); nothing is computed on the CPU. */
struct quisk_cFilter {                      /* filter.h:1-10 */
    double *dCoefs;
    double *cpxCoefs;                       /* complex double * */
    int nBuf;
    int nTaps;
    int decim_index;
    double *cSamples;                       /* complex double *, nTaps entries */
    double *ptcSamp;                        /* next write position inside cSamples */
    double *cBuf;
};
struct quisk_cHB45Filter {                  /* filter.h:23-29 */
    double *cBuf;
    int nBuf;
    int toggle;
    double samples[2 * 22];                 /* complex double samples[22] */
    double center[2 * 11];                  /* complex double center[11]  */
};
void quisk_filt_cInit(struct quisk_cFilter *filter, double *coefs, int taps);               /* filter.c:9-20 */
void quisk_filt_tune(struct quisk_cFilter *filter, double freq, int ssb_upper);             /* filter.c:58-81 */
int quisk_cDecimate(double *cSamples, int count, struct quisk_cFilter *filter, int decim);  /* filter.c:203-229 */
int quisk_cCDecimate(double *cSamples, int count, struct quisk_cFilter *filter, int decim); /* filter.c:231-257 */
int quisk_cFilter(double *cSamples, int count, struct quisk_cFilter *filter);               /* filter.c:372-375 */
int quisk_cDecim2HB45(double *cSamples, int count, struct quisk_cHB45Filter *filter);       /* filter.c:377-417 */
/* struct quisk_dFilter (filter.h:12-21) has the layout of struct quisk_cFilter; its history ring holds doubles. */
struct quisk_dHB45Filter {                  /* filter.h:31-37 */
    double *dBuf;
    int nBuf;
    int toggle;
    double samples[22];
    double center[11];
};
void quisk_filt_dInit(struct quisk_cFilter *filter, double *coefs, int taps);               /* filter.c:22-33 */
void quisk_filt_differInit(struct quisk_cFilter *filter, int taps);                         /* filter.c:35-56 */
int quisk_cInterpolate(double *cSamples, int count, struct quisk_cFilter *filter, int interp);      /* filter.c:131-165 */
int quisk_dInterpolate(double *dSamples, int count, struct quisk_cFilter *filter, int interp);      /* filter.c:167-201 */
int quisk_cInterpDecim(double *cSamples, int count, struct quisk_cFilter *filter, int interp, int decim);  /* filter.c:287-324 */
int quisk_dDecimate(double *dSamples, int count, struct quisk_cFilter *filter, int decim);  /* filter.c:259-285 */
int quisk_dFilter(double *dSamples, int count, struct quisk_cFilter *filter);               /* filter.c:347-370 */
double quisk_dD_out(double sample, struct quisk_cFilter *filter);                           /* filter.c:326-345 */
int quisk_cInterp2HB45(double *cSamples, int count, struct quisk_cHB45Filter *filter);      /* filter.c:455-488 */
int quisk_dInterp2HB45(double *dSamples, int count, struct quisk_dHB45Filter *filter);      /* filter.c:420-453 */
/* quisk_dC_out (filter.c:83-104) returns `complex double` by value.  The library exports it under the reference's own name
 * (microphone.c:469 links against it unchanged); ISO C++ has no spelling for the type, so the declaration is for C translation
 * units, and qh_quisk_dC_out is the same computation with the result written through a pointer. */
#ifndef __cplusplus
double _Complex quisk_dC_out(double sample, struct quisk_cFilter *filter);
#endif
void qh_quisk_dC_out(double sample, struct quisk_cFilter *filter, double *out_re_im);

#ifdef __cplusplus
}
#endif
#endif
