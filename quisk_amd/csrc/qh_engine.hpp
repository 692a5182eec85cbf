// qh_engine.hpp -- the batched RXA receive engine for MI355X: its constants, the channels' settings (ChanCfg; the notes of pending work
// apart in ChanCfg::Work), the engine's state (Engine; the engine-wide settings apart in Engine::Wide) and the handle of the C ABI.
// A new dsp_rate or dsp_size (Engine::rebuild) keeps ChanCfg's direct members and Wide and starts everything else again.  Declarations only: qh_engine.hip launches, qh_engine_params.hip designs, allocates and uploads,
// qh_rxa_api.hip is the C ABI.  Besides alloc / grow / put_row and one-line accessors no function is defined here, and no ABI function.
//
// Mirrors create_rxa()/xrxa() of the reference (wdsp/RXA.c:31-598) for the blocks on the hot path.
// Per-channel differences are data (NCO step, masks, 2x2 output matrix), not control flow, so one
// launch per stage covers every channel:
//
//   front   : xshift + xresample(in)      -> qh::osfir_kernel<NFFT, D = in_rate/dsp_rate, MIX>
//   nbp0    : xnbp (fircore)              -> qh::osfir_kernel<NFFT, 1>
//   bp1     : xbandpass (fircore)         -> qh::osfir_kernel<NFFT, 1>      (only when some channel runs it)
//   epilogue: xwcpagc mode 0 + xpanel     -> fused into the last launch (2x2 real matrix per channel)
//
// State carried between calls (all device resident, right-aligned rows of the most recent samples):
//   hist_front [2][nch][HF]  raw input samples (the reference's resampler ring holds them behind xshift; here the
//                            oscillator sits behind the filter, qh_osfir.hpp OUTMIX, and nco_retune_hist_kernel
//                            rewrites the row when a channel's shift changes)
//   fc[s].hist [2][nch][HB]  the input samples of fircore stage s (the reference's fircore delay line)
//   nco_phase  [nch]         64-bit fixed-point turns
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/quiskhip.h"
#include "qh_design.hpp"
// the stage headers, for the parameter and state types held by value; each of their `static` kernels is launched by one unit only
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "qh_kernels.hpp"
#include "qh_demod.hpp"
#include "qh_tiled.hpp"
#include "qh_agc_tiled.hpp"
#include "qh_emnr.hpp"
#include "qh_snba.hpp"
#include "qh_audio_peak.hpp"
#include "qh_ssql.hpp"
#include "qh_fmsq.hpp"
#include "qh_taps.hpp"
#include "qh_gen.hpp"
#pragma clang diagnostic pop
#include "qh_internal.hpp"

namespace qh {

static constexpr int kNfft = 4096;          // FFT size of the front stage and, for nc <= 2048, of the fircore stages
static constexpr int kBandNfftMax = 8192;   // fircore stages with 2048 < nc <= 4096 run 8192-point tiles (Engine::bnfft)
static constexpr int kHistBand = 4095;      // fircore history capacity: nc up to 4096
// nc = 8192 ... 65536 (RXASetNC, wdsp/RXA.c:934-946): the impulse response in partitions of 4096 taps, every partition an ordinary
// 8192-point tile pass over a view of the stream that starts 4096 p samples earlier, the passes added (Engine::run_band)
static constexpr int kLongPart = 4096, kLongNcMax = 65536, kLongParts = kLongNcMax / kLongPart, kLongHist = kLongNcMax - 1;
static constexpr int kHistFront = 2240;     // resampler history capacity: 140 * D taps, D <= 16
// FM PLL time tiles (qh_tiled.hpp).  On a carrier the loop (double pole at 0.66 per sample) forgets its start state in ~100
// samples; on noise alone two runs meet after ~135 samples on average with an exponential tail, so a 768-sample warm-up
// leaves a fraction of a percent of the tiles to the verify kernel's sequential re-run.
static constexpr int kFmTile = 256;        // shortest tile; long calls take up to 2048 samples per lane (Engine::process_chain)
static constexpr int kFmWarm = 768;
// SAM's loop (omega_N 250 rad/s, zeta 1, RXA.c:185-186) forgets a state in exp(-250 t): 1e-16 after 0.147 s = 7068 samples at 48 kHz
static constexpr int kSamTile = 4096;
static constexpr int kSamWarm = 8192;
static constexpr long long kSamTiledMin = 4 * 8192;     // shorter calls take the sequential kernel
static constexpr int kAgcSegs = 16;                     // super-segments of the AGC boundary pass, at most
static constexpr long long kAgcTiledMin = 16384;        // xwcpagc in time tiles from this many detector samples per call (qh_agc_tiled.hpp)

struct ChanCfg {
    int mode = QH_LSB;                                          // RXA.c:33
    int shift_run = 1; double shift_freq = 0.0;                 // RXA.c:39-45
    int nbp_run = 1, nbp_nc = 2048, nbp_wintype = 0;            // RXA.c:90-106
    // minimum-phase impulse responses, one flag per fircore as in the reference (RXANBPSetMP nbp.c:578, SetRXABandpassMP bandpass.c:447,
    // RXABPSNBASetMP snb.c:844); RXASetMP (RXA.c:948) writes all of them
    int nbp_mp = 0, bp1_mp = 0, snb_mp = 0;
    // notch database (create_notchdb RXA.c:85-87) and nbp0's use of it (fnfrun 0, autoincr 1: RXA.c:92,104)
    std::vector<Notch> notches;
    double ndb_tunefreq = 0.0, ndb_shift = 0.0;
    int fnfrun = 0, autoincr = 1;
    double nbp_flow = -4150.0, nbp_fhigh = -150.0, nbp_gain = 1.0;
    int amd_run = 0, amd_mode = 0, fmd_run = 0;                 // RXA.c:175-212
    int agc_run = 1, agc_mode = 3; double agc_fixed = 1000.0;   // RXA.c:335-358
    double agc_tau_attack = 0.001, agc_tau_decay = 0.250, agc_max_gain = 10000.0, agc_var_gain = 1.5;
    double agc_hangtime = 0.250, agc_hang_thresh = 0.250;
    double agc_max_input = 1.0;                                 // SetRXAAGCMaxInputLevel, wcpAGC.c:550-557
    bool agc_on() const { return agc_run && agc_mode != 0; }
    int bp1_run = 1, bp1_nc = 2048, bp1_wintype = 1;            // RXA.c:377-389
    double bp1_flow = -4150.0, bp1_fhigh = -150.0, bp1_gain = 1.0;
    double gain1 = 4.0, gain2I = 1.0, gain2Q = 1.0;             // RXA.c:464-474
    int inselect = 3, copy = 0;
    int levelfade = 1, sbmode = 0;                              // RXA.c:180-181
    double fm_dev = 5000.0, ctcss_freq = 254.1;                 // RXA.c:198,208
    int ctcss_run = 1;                                          // RXA.c:207
    // xfmd's de-emphasis and audio filters (create_fmd's arguments, RXA.c:209-212: nc max(2048, dsp_size) -- Engine::init --, mp 0; the
    // audio band, RXA.c:196-197)
    int fm_nc_de = 2048, fm_mp_de = 0, fm_nc_aud = 2048, fm_mp_aud = 0;
    double fm_f_low = 300.0, fm_f_high = 3000.0;
    int lim_run = 0; double lim_gain = 2.5;                     // FM detector limiter, fmd.c:106-108
    // anf / anr (create_anf / create_anr of create_rxa, RXA.c:278-315): [0] = anf, [1] = anr
    struct Lms { int run = 0, position = 0, taps = 64, delay = 16; double two_mu = 0.0001, gamma = 0.1; } lms[2];
    // emnr (create_emnr of create_rxa, RXA.c:319-332)
    // snba (wdsp/snb.c) and its bandpass bpsnba (snb.c:696-855; run / position follow the mode, RXA.c:883-917)
    int snba_run = 0;
    int snb_nc = 2048;                                          // bpsnba's own nc (RXABPSNBASetNC, snb.c:829-842; made with nbp0's, RXA.c:114)
    double snba_f_low = 200.0, snba_f_high = 0.0;               // outresamp fc_low / fcin (snb.c:45-46, resample.c:195-204)
    int snb_pos() const {
        if (!snba_run) return -1;
        switch (mode) {
        case QH_LSB: case QH_CWL: case QH_DIGL: case QH_USB: case QH_CWU: case QH_DIGU: return 0;
        case QH_AM: case QH_SAM: case QH_DSB: case QH_FM: return 1;
        default: return -1;
        }
    }
    int emnr_run = 0, emnr_pos = 0, emnr_gain_method = 2, emnr_npe = 0, emnr_ae = 1;
    double emnr_ae_zeta = 0.75, emnr_ae_psi = 20.0, emnr_train_zeta = -2.0, emnr_train_t2 = 0.20;       // emnr.c:332,491-493
    // amsq (create_amsq of create_rxa, RXA.c:158-172)
    int amsq_run = 0; double amsq_tail_thresh = 0.009, amsq_unmute_thresh = 0.010, amsq_max_tail = 1.5;
    int bp1_pos = 0;                                            // SetRXAANFPosition / SetRXAANRPosition set it too (anf.c:236)
    // xcbl, xspeak, xmpeak (create_rxa, RXA.c:403-445: all three made with run 0); the design setters zero their cascade (w.sp_flush,
    // w.mp_flush) at the next block boundary
    int cbl_run = 0, sp_run = 0, mp_run = 0, mp_npeaks = 2;
    double sp_f = 600.0, sp_bw = 100.0, sp_gain = 2.0;
    int mp_enable[kApPeaks] = { 1, 1 };
    double mp_f[kApPeaks] = { 2125.0, 2295.0 }, mp_bw[kApPeaks] = { 75.0, 75.0 }, mp_gain[kApPeaks] = { 1.0, 1.0 };
    bool ap_on() const { return cbl_run || sp_run || mp_run; }
    // xssql (create_ssql of create_rxa, RXA.c:447-461: run 0, wthresh 0.08, tau_mute = tau_unmute = 0.1); no setter flushes it
    int ssql_run = 0;
    double ssql_wthresh = 0.08, ssql_tau_mute = 0.1, ssql_tau_unmute = 0.1;
    bool ssql_on() const { return ssql_run != 0; }
    // xfmsq (create_fmsq of create_rxa, RXA.c:214-234: run 0, tail 0.750, unmute 0.562 -- not 0.9 apart until SetRXAFMSQThreshold runs --,
    // nc max(2048, dsp_size), mp 0)
    int fmsq_run = 0, fmsq_nc = 2048, fmsq_mp = 0;
    double fmsq_tail_thresh = 0.750, fmsq_unmute_thresh = 0.562;
    // xeqp (create_eqp of create_rxa, RXA.c:257-275: run 0, nc max(2048, dsp_size) -- Engine::init --, mp 0, ten frequencies with 0 dB each,
    // ctfmode 0, wintype 0).  eqp_F / eqp_G: nfreqs + 1 entries, G[0] the preamp, F[0] not read
    int eqp_run = 0, eqp_nc = 2048, eqp_mp = 0, eqp_ctfmode = 0, eqp_wintype = 0;
    std::vector<double> eqp_F = { 0.0, 32.0, 63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 16000.0 }, eqp_G = std::vector<double>(11, 0.0);
    // xsender / xsiphon (qh_taps.hpp): both off until enabled -- a tap costs a pass (the reference runs the siphon of every channel,
    // RXA.c:392-401, and the sender of channel 0, RXA.c:131)
    int sender_run = 0, sip_run = 0;
    // gen0 (qh_gen.hpp) as create_rxa makes it (RXA.c:60-66: run 0, mode 2) with create_gen's defaults (gen.c:113-152); the two-tone and
    // pulse settings have no RXA setter.  gen_seed_set: qh_rxa_set_gen_seed has replaced the default seed, a fixed function of the channel.
    int gen_run = 0, gen_mode = 2;
    double gen_tone_mag = 1.0, gen_tone_freq = 1000.0, gen_noise_mag = 1.0;
    double gen_sweep_mag = 1.0, gen_sweep_f1 = -20000.0, gen_sweep_f2 = 20000.0, gen_sweep_rate = 4000.0;
    unsigned long long gen_seed = 0;
    bool gen_seed_set = false;
    // The notes of work: what a setter has left for the next call to do (dirty: design and upload again; flush: zero that state) and what
    // is on the device now.  The rule for a new member of ChanCfg: a note of work goes in Work; anything that a setter list replayed on
    // a fresh engine would reproduce is a setting and goes outside.  Engine::rebuild keeps the settings and starts Work from its defaults.
    struct Work {
        int shift_on_device = 1;            // whether the device phase is live or parked (nco_park_kernel)
        bool agc_dirty = true;
        int agc_abuf = -1;                  // attack_buffsize last uploaded
        bool agc_rewindow = false;          // the attack window moved in mid-stream: the state's ring is taken again from the full one
        bool agc_ran = false, agc_stale = false;    // the window moved while the ring held samples: ring_max may be stale (qh_agc_tiled.hpp)
        struct Lms { bool dirty = true, flush = false; } lms[2];
        bool snba_flush = false, snba_taps_dirty = true, snba_rout_flush = false, snb_dirty = true, snb_flush = false;
        bool emnr_dirty = true, emnr_flush = false, amsq_dirty = true;
        bool demod_dirty = true, ctcss_flush = false;
        bool nbp_dirty = true, bp1_dirty = true, nco_dirty = true, epi_dirty = true;
        bool nbp_flush = false, bp1_flush = false;
        bool ap_dirty = true, sp_flush = false, mp_flush[kApPeaks] = { false, false };
        bool ssql_dirty = true, fmsq_dirty = true, lim_dirty = true;
        bool fm_de_flush = false, fm_aud_flush = false;     // SetRXAFMNCde / NCaud took a new nc (setNc_fircore zeroes that filter's line)
        // eqp_flush: SetRXAEQNC took a new nc (setNc_fircore zeroes the delay line); eqp_tie: two frequencies coincide after eq_impulse's
        // clamp at this dsp_rate while their gains differ
        bool eqp_dirty = true, eqp_flush = false, eqp_tie = false;
        bool gen_dirty = true, gen_sweep_dirty = true, gen_tone_reset = false, gen_sweep_reset = false;
    } w;
    // xwcpagc mode 0 with a position-1 stage behind it: the gain is applied in place at the AGC's spot, not in the epilogue
    // (the new stages sit behind xwcpagc too, ahead of the panel: a fixed gain that changes while a peak still rings must not reach
    // the ringing tail, so it is applied at the AGC's spot for them as well; SSQL's detector reads amplitude, so it needs the gain too)
    bool fix_before() const
    {
        return agc_run && agc_mode == 0 && ((bp1_run && bp1_pos) || (lms[0].run && lms[0].position) || (lms[1].run && lms[1].position) ||
                                            (emnr_run && emnr_pos) || ap_on() || ssql_on());
    }
};

// The overlap-save "fircore" stages of the chain (wdsp/firmin.c), in the order of their ping-pong bits in Engine::flags():
// nbp0, bp1, the FM de-emphasis and audio filters, bpsnba, xfmsq's noise filter, xeqp
enum FcId { FC_NBP, FC_BP1, FC_DE, FC_AUD, FC_SNB, FC_FQ, FC_EQP, FC_COUNT };

// One fircore stage: its mask rows, its delay lines and where each channel's line lies.
// The delay lines are a ping-pong pair [2][nch][kHistBand]: a launch reads half `cur` and writes the other one for its own channels, and
// the pair flips once per call in which the stage ran (flip(): the callers' step, so that one call may run the stage over several
// channel lists).  A fircore keeps its delay line while its channel sits the stage out (xbandpass / xnbp / xeqp with run 0 only copy),
// so a channel that is not listed keeps its rows in the half that was current when it left: chan[ch].at (Engine::fc_follow).
// Long impulse responses (nc > 4096, kLongPart): `parts` partitions (1: the ordinary path), their masks lmask ([nch or 1][kLongParts][8192]),
// how many of them each mask row's own impulse response reaches lrow_parts ([nch or 1]) and the stage's last kLongHist input samples
// lhist [2][nch][kLongHist].  can_long: xfmsq's noise filter and xeqp never take that form (Engine::chain_needs refuses such an nc).
struct Fircore {
    double2 *mask = nullptr;
    long long mask_stride = 0;              // kBandNfftMax: one mask row per channel; 0: one row shared by the stage's channels
    // The FM de-emphasis and audio filters hold one mask row per distinct design among their running channels (Engine::fm_filters):
    // by_design, `rows` of them allocated.  One row: mask_stride 0 and no mask_row, the shared row of old; more: mask_stride
    // kBandNfftMax and mask_row [nch], the row of every channel (OsfirArgs::mask_row).  lmask / lrow_parts go by the same rows.
    bool by_design = false;
    int rows = 1;
    int *mask_row = nullptr;
    long long mask_rows(int nch) const { return by_design ? rows : mask_stride ? nch : 1; }
    double2 *hist[2] = { nullptr, nullptr };
    int cur = 0;
    bool ChanCfg::Work::*dirty = nullptr;   // nbp0, bp1, bpsnba: the channel's flag that has its mask row designed and uploaded again (plan_long)
    bool can_long = true;
    int parts = 1;
    double2 *lmask = nullptr, *lhist[2] = { nullptr, nullptr };
    int *lrow_parts = nullptr;
    // listed: the channel ran the stage when its lists were last made; at: the half that holds its rows; long_live: it has run the stage
    // with nc > 4096 since RXASetNC last zeroed its lines, so it holds more than the one-tile form has room for (Engine::plan_long)
    struct Chan { bool listed = false, long_live = false; int at = 0; };
    std::vector<Chan> chan;
    // Engine::rebuild has put the delay lines the stage held before a change of the DSP rate in place (setImpulse_fircore(..., 1) keeps
    // them, firmin.c:449-453): the fc_alloc that makes the stage keeps them and the rows' places, once
    bool carried = false;
    void flip() { cur ^= 1; }
};

struct Engine {
    int device = 0, nch = 0, dsp_size = 0, in_rate = 0, dsp_rate = 0, out_rate = 0;
    int D = 1, dsp_insize = 0, dsp_outsize = 0, front_fold = 1, front_pick = 1;
    unsigned long long epoch = 0;       // bumped by every setter / flush: a captured launch sequence is stale when it moves
    // Launch-sequence replay (qh_rxa_set_graph_replay): a process() call whose arguments and parameters repeat is
    // captured into a hipGraph, one per state of the ping-pong history flags, and replayed.  Everything the host
    // side of process() changes from call to call is those flags, so a slot also records the flags it leaves behind.
    struct GraphKey {
        const void *in = nullptr; void *out = nullptr; long long in_stride = 0, out_stride = 0; int nblk = 0;
        unsigned long long epoch = ~0ull;
        bool operator==(const GraphKey &o) const
        { return in == o.in && out == o.out && in_stride == o.in_stride && out_stride == o.out_stride && nblk == o.nblk && epoch == o.epoch; }
    };
    struct GraphSlot { hipGraphExec_t exec = nullptr; unsigned after = 0; };
    // The engine-wide settings.  The rule for a new member of Engine: a value that is set through the C ABI outside cfg and must outlive
    // a rebuild (a new dsp_rate or dsp_size) lives here; Engine::rebuild moves `wide` out and back as a whole and carries nothing else
    // of this kind.  (eg, pk and pk_src are set for one call and are not settings.)
    struct Wide {
        bool graph_on = false;                  // qh_rxa_set_graph_replay
        bool timing = false, meters_on = false;
        int band_tile_pref = 0;                 // qh_rxa_set_band_tile: 0 / 4096: 4096-point tiles, 8192: the two-group tiles
        int snba_ovrlp = 4;                     // create_rxa's overlap (RXA.c:244): incr = xsize / 4
        int snba_form = 0;                      // qh_rxa_set_snba_form (the blanker's two forms, below)
        std::vector<SnbaTune> snba_tune_h;      // [nch]: the blanker's tuning, uploaded to snba_tune when a tuning setter has run
        // a display bank fed from the sender rows at the end of every call (qh_rxa_attach_display)
        qh_ana *disp = nullptr;
        int disp_ss = 0;
        int pll_check_only = 0;                 // diagnostics (qh_rxa_debug_pll): count unconverged tiles without re-running them
        int agc_form = 0;                       // diagnostics (qh_rxa_debug_agc): 1 = the sample-by-sample form of the wcpAGC loop
        bool emnr_tables = false;               // qh_rxa_SetEMNRTables has run: the tables below
        std::vector<double> h_GG, h_GGS, h_zeta; std::vector<int> h_zeta_true; double h_zrange[4] = { 0, 0, 0, 0 };
    } wide;
    bool graph_seen = false;
    GraphKey graph_key;
    GraphSlot graph_slot[256];
    long long graph_launches = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // the AM / SAM detectors of a call run beside the FM detector chain: other channels' rows, other state (process_chain)
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<ChanCfg> cfg;
    // front (resampler) design
    int front_ntaps = 0, front_P = 0, front_L = 0;
    // device state
    double2 *mask_front = nullptr;
    double2 *tw4096 = nullptr, *tw_inv_front = nullptr, *tw8192 = nullptr;
    int bnfft = kNfft;                      // tile size of the fircore stages: what their masks are built for (4096 or 8192)
    bool band2g = false;                    // 8192-point tiles shared by two lane groups (osfir8k_kernel): masks stored [even | odd]
    bool band6k = false;                    // 6144-point tiles on 384 lanes (osfir6k_kernel)
    int dbg_forms = [] { const char *e = std::getenv("QH_DBG_FORMS"); return e ? std::atoi(e) : 0; }();   // see process_chain
    std::vector<cd> band_mask(const std::vector<cd> &h) const;
    unsigned long long *nco_phase = nullptr, *nco_dphase = nullptr, *nco_parked = nullptr;
    double2 *nco_step = nullptr;
    // output-side oscillator of the front stage (D > 1): per-channel lane table, per-launch tile table, the resampler taps,
    // and the scratch lists of refresh_params (channel list, new phase law)
    double2 *lane_rot = nullptr, *tile_rot = nullptr;
    long long tile_rot_cap = 0;             // tiles per channel
    double *front_taps = nullptr;
    int *retune_list = nullptr;
    unsigned long long *retune_law = nullptr;
    EpiParam *epi = nullptr;
    double2 *hist_front[2] = { nullptr, nullptr };
    int cur_front = 0;
    Fircore fc[FC_COUNT];
    double2 *buf[2] = { nullptr, nullptr };
    long long buf_cap = 0;                  // complex samples per channel
    // long impulse responses (Fircore::parts > 1): lcat: history + block of the stage being run, ltmp: a partition's output
    double2 *lcat = nullptr, *ltmp = nullptr;
    long long lcat_cap = 0;                 // the buf_cap they were made for
    int long_stage_alloc(Fircore &f);
    int long_buffers();
    int long_masks_upload(Fircore &f, long long row, const std::vector<cd> &h);
    // Every device buffer the engine owns, by its address, and its size in bytes: alloc() enters it, ~Engine frees it, dev_bytes()
    // adds them up (the qh_rat resamplers hold their own)
    std::map<void *, long long> owned;
    long long dev_bytes() const { long long b = 0; for (const auto &o : owned) b += o.second; return b; }
    // timing (wide.timing)
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_cat;
    int ev_used = 0;
    double last_ms[3] = { 0, 0, 0 };

    // demodulators (allocated on first use)
    bool demod_alloc = false, lists_dirty = true;
    // The channel lists of the mixed-mode chain, one device block for all of them (build_lists): every list has nch slots, the
    // pair lists 2 nch.  [L_LMS + 3 f + k]: anf (f = 0) / anr (f = 1) at position 0 (k = 0, always in `cur`) or at position 1 with
    // the data in cur (k = 1: bp1 still to come or not running) or in other (k = 2: bp1 ran at position 0); L_EMNR likewise.
    // [L_BP1P + p]: bp1 at position p.  [L_FIX + b], [L_AP + b], [L_AGC_CUR / OTHER]: by the buffer (0 cur, 1 other) that holds the
    // channel at that stage.  [L_SNB + p]: bpsnba at position p.
    enum ListId {
        L_AM, L_SAM, L_FM, L_BP1, L_PLAIN, L_AGC_CUR, L_AGC_OTHER, L_LMS, L_BP1P = L_LMS + 6, L_FIX = L_BP1P + 2, L_AMSQ = L_FIX + 2, L_EMNR,
        L_SNB = L_EMNR + 3, L_SNBA = L_SNB + 2,
        L_REST,             // the channels that are not FM (the mixed-mode path runs the two kinds on two streams) ...
        L_USB, L_RB,        // ... those of them without / with a bp1 stage
        L_LIM, L_AP, L_PAIRS_FM = L_AP + 2, L_PAIRS_AM, L_PAIRS_SAM, L_COUNT
    };
    struct ChanList { int *dev = nullptr; int n = 0; };
    ChanList lists[L_COUNT];
    // The channel lists of a stage that is made on first use: R rows of nch slots in one device block of their own (an engine that never
    // runs the stage allocates nothing for it), row r's slots and count in row[r] (also lists[r]) and its channels on the host in h[r].
    // list_make allocates the block (through alloc(), so `owned` holds it; the caller has quiesced) and points the rows into it;
    // list_upload copies the host rows, each padded with zeros to nch, into it on `stream` -- `image` is that copy's source, kept here
    // because the copy is not waited for -- and does nothing while the block has not been made.
    template <int R> struct ListBlock {
        int *block = nullptr;
        ChanList row[R];
        std::vector<int> h[R], image;
        const ChanList &operator[](int r) const { return row[r]; }
        bool any() const { for (const ChanList &l : row) if (l.n) return true; return false; }
        void clear() { for (std::vector<int> &v : h) v.clear(); }
        void count() { for (int r = 0; r < R; r++) row[r].n = (int)h[r].size(); }
    };
    template <int R> int list_make(ListBlock<R> &b);
    template <int R> int list_upload(ListBlock<R> &b);
    int *list_block = nullptr;
    // channel pairs for the real filters behind the detectors (osfir_kernel PAIR): FM de-emphasis, bp1 of the AM and of the SAM channels
    // (partners have the same design; bp1: count 0 when a channel of the kind has complex taps; FM: de_real says that no running
    // channel's de-emphasis row has one)
    int np_fm = 0, np_am = 0, np_sam = 0;
    bool de_real = false;
    bool all_nbp = false;
    int n_sam0 = 0;                         // the first n_sam0 entries of lists[L_SAM] have sbmode 0 (no all-pass chains): time-tiled in long calls
    // xwcpagc mode 0 ahead of a position-1 anf / anr / bp1: the fixed gain does not commute with what follows when it
    // changes, so it is applied where the reference applies it (lists[L_FIX + b])
    double *fix_gain = nullptr;
    // xcbl / xspeak / xmpeak (qh_audio_peak.hpp), made when a channel first runs one of them: parameters, state [nch][kApW], the carry
    // matrices T = A^ap_L [nch][kApDim^2] and the tiles' end / start states [nch][ap_ends_cap][kApW]
    ApParam *ap_prm = nullptr;
    double *ap_state = nullptr, *ap_M = nullptr, *ap_ends = nullptr;
    long long ap_ends_cap = 0;
    int ap_L = 0;
    std::vector<double> ap_M_h;
    std::vector<ApParam> ap_prm_h;
    int ap_alloc();
    // xssql (qh_ssql.hpp), made when a channel first runs it: its two channel lists (by the buffer that holds the row, as L_AP),
    // parameters, state, the ramps, the tiles' rows
    // [nch][ssql_ends_cap][kSsE], the crossing / window / trigger bits [3][nch][ssql_wcap] and the words' machine records [nch][ssql_wcap]
    ListBlock<2> ssql_lists;
    SsqlParam *ssql_prm = nullptr;
    SsqlState *ssql_state = nullptr;
    double *ssql_cup = nullptr, *ssql_cdown = nullptr, *ssql_ends = nullptr;
    unsigned long long *ssql_bits = nullptr;
    int *ssql_rec = nullptr;
    long long ssql_ends_cap = 0, ssql_wcap = 0, ssql_rec_cap = 0;
    int ssql_L = 0, ssql_ntup = 0, ssql_ntdown = 0;
    std::vector<SsqlParam> ssql_prm_h;
    int ssql_alloc();
    // xfmsq (qh_fmsq.hpp), made when a channel first runs it, in blocks of its own: the list of its channels [0] and their pairs for the
    // noise filter [1] (neighbours in the list, np_fq of them; an odd channel out is its own partner, so up to nch + 1 entries: they
    // run on into the third row, which holds nothing else), parameters, state, the ramps, the noise filter (fc[FC_FQ]: one design for
    // the engine's FMSQ channels) and its output rows [nch][fq_noise_cap]
    ListBlock<3> fq_lists;
    int np_fq = 0;
    FmsqParam *fq_prm = nullptr;
    FmsqState *fq_state = nullptr;
    double *fq_cup = nullptr, *fq_cdown = nullptr;
    double2 *fq_noise = nullptr;
    long long fq_noise_cap = 0;
    int fq_ntup = 0, fq_ntdown = 0, fq_nready = 0, fq_nc_built = 0, fq_mp_built = 0, fq_key_built = 0;
    int fmsq_alloc();
    int prm_fmsq(ChanCfg &c, int ch);
    int fmsq_filter();
    void launch_fmsq_flush();
    // xeqp (wdsp/eq.c:166-208), made when a channel first runs it, in blocks of their own: the list of its channels [0] and of the others
    // [1] (the linear path passes those on in a pointwise pass; counted as none until the stage exists) and fc[FC_EQP], one mask row per
    // channel (EQ profiles are per channel, as bp1's designs)
    ListBlock<2> eq_lists;
    std::vector<std::vector<cd>> eq_taps_h;     // per channel: the taps behind the mask row last uploaded (qh_rxa_debug_eqp); empty until then
    int eq_key_built = 0;
    bool eq_lists_dirty = false;
    std::vector<cd> eqp_taps(const ChanCfg &c) const;
    int eqp_alloc();
    int refresh_eqp();
    // xsender / xsiphon (qh_taps.hpp), made when a channel first runs one of them, in blocks of their own: the lists of their channels
    // ([0] the sender's; [1] / [2] the siphon's by the buffer that holds the row behind bp1, as L_AP), the sender's float rows of the last
    // call [nch][snd_cap] (snd_n samples each), the siphon's rings [nch][kSipSize] with their write indices [nch], and per channel the
    // fixed AGC gain that the output matrix applies behind the siphon's point (1.0 where it does not: refresh_params)
    ListBlock<3> tap_lists;
    float2 *snd_rows = nullptr;
    long long snd_cap = 0, snd_n = 0;
    double2 *sip_ring = nullptr;
    int *sip_idx = nullptr;
    double *tap_gain = nullptr;
    int taps_alloc();
    // gen0 (qh_gen.hpp), made when a channel first runs it: the list of its channels, their parameters and state, the sweep tables
    // [nch][kGenCkMax] and the pulse's raised-cosine edge [pntrans + 1] (calc_pulse, gen.c:88-95)
    ListBlock<1> gen_lists;
    GenParam *gen_prm = nullptr;
    GenState *gen_state = nullptr;
    double2 *gen_ck = nullptr;
    double *gen_ctrans = nullptr;
    std::vector<GenParam> gen_prm_h;
    int gen_pntrans = 0, gen_pnon = 0, gen_pnoff = 0;
    int gen_alloc();
    int prm_gen(ChanCfg &c, int ch);
    int refresh_gen();
    // the attached display (wide.disp): disp_fed is recorded on the bank's stream behind its append of the rows and waited for by the
    // engine's stream ahead of the next call's launches
    hipEvent_t disp_fed = nullptr;
    bool disp_fed_pending = false;
    int feed_display(qh_ana *a, int ss);
    int process_fed(bool replay, const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk);
    // snba: the blanker's parameters, taps, state and the Toeplitz-inverse scratch
    SnbaParam snba_prm{};
    double *snba_state = nullptr, *snba_hin = nullptr, *snba_hout = nullptr, *snba_scratch = nullptr;
    SnbaIdx *snba_idx = nullptr;
    SnbaTune *snba_tune = nullptr;          // [nch]; host copy wide.snba_tune_h, uploaded when a tuning setter has run
    bool snba_tune_dirty = true;
    int snba_alloc();
    void snba_plan(int ovrlp);
    int snba_set_ovrlp(int ovrlp);
    // The blanker's two forms (qh_snba.hpp).  qh_rxa_set_snba_form: 0 = the single kernel where it can run (dsp_rate up to 48 kHz and
    // dsp_size up to 1024) and the three passes elsewhere, 1 = the three passes everywhere.  The state is one layout for both, so the
    // form (wide.snba_form) may change between calls.  snba_r12: the passes' 12 kHz rows, [2][nch][snba_r12_cap] (into the frames | out of them).
    double *snba_r12 = nullptr;
    long long snba_r12_cap = 0;
    bool snba_rows() const { return wide.snba_form == 1 || snba_prm.ratio > kSnbFusedMaxRatio || dsp_size > kSnbFusedMaxDsp; }
    // the dsp_rate / dsp_size pairs the blanker takes: 12000 * 2^k (k = 0 .. 5), the size a multiple of the ratio and at most 4096
    static bool snba_accepts(int rate, int size);
    static const char *snba_accepted() { return "SNBA: dsp_rate 12000, 24000, 48000, 96000, 192000 or 384000 and dsp_size a multiple of dsp_rate / 12000, up to 4096"; }
    EmnrParam emnr_prm{};
    EmnrChan *emnr_chan = nullptr;
    EmnrScalars *emnr_scal = nullptr;
    double *emnr_state = nullptr, *emnr_window = nullptr, *emnr_GG = nullptr, *emnr_GGS = nullptr, *emnr_zeta = nullptr;
    int *emnr_zeta_true = nullptr;
    AmsqParam *amsq_prm = nullptr;
    AmsqState *amsq_state = nullptr;
    double *amsq_cup = nullptr, *amsq_cdown = nullptr, *amsq_mag = nullptr;
    long long amsq_mag_cap = 0;
    int amsq_ntup = 0, amsq_ntdown = 0;
    LmsParam *lms_prm[2] = { nullptr, nullptr };
    LmsState *lms_state[2] = { nullptr, nullptr };
    // The long form of anf / anr (lms_long_kernel: more than 64 taps, or a delay of 0 or above 64).  lists[L_LMS + 3 f + k] holds the
    // short-form channels alone and lms_long_lists[3 f + k] the others, in a block of their own made with the first of them (an engine
    // without one allocates what it did before); lms_long_Ks: bit log2(K) set when a channel of the list runs at K taps per lane.
    // lms_long_rows[f]: weights and ring [nch][kLmsLongRow], made when filter f first has such a channel.
    ListBlock<6> lms_long_lists;
    unsigned lms_long_Ks[6] = { 0, 0, 0, 0, 0, 0 };
    double *lms_long_rows[2] = { nullptr, nullptr };
    static bool lms_long_form(const ChanCfg::Lms &m) { return m.taps > 64 || m.delay < 1 || m.delay > 64; }
    int lms_n(int k) const { return lists[L_LMS + k].n + lms_long_lists[k].n; }       // channels of either form on LMS list k
    int *levelfade = nullptr;
    AmState *am_state = nullptr;
    // carries of the grid-segmented scans (qh_tiled.hpp: a launch reads the state of its channels and leaves the new one here; a
    // commit kernel behind it moves it in): [nch] each
    AmState *am_next = nullptr;
    SnotchState *sn_next = nullptr;
    double *fmdc_next = nullptr;
    double *fm_cin = nullptr, *fm_pw = nullptr;       // xfmd's dc removal taken in the de-emphasis stage's load: fmdc ahead of every tile, mtau^(k + 1)
    long long fm_cin_cap = 0;
    struct FmDcSrc { const double *a; long long stride; int shift; } ;
    const FmDcSrc *band_fmdc = nullptr;               // set around the run_band call of that stage
    double *am_cin = nullptr, *am_pw = nullptr, *am_last = nullptr;      // the fade leveller's carried share taken in bp1's load (osfir_kernel DET 3)
    long long am_cin_cap = 0;
    const FmDcSrc *band_amlv = nullptr;
    AmParam am_prm{};
    PllState *pll_state = nullptr;          // the SAM detector's loop (amd.c) ...
    PllState *fm_pll_state = nullptr;       // ... and the FM detector's (fmd.c): two objects in the reference, each keeps its state while the other runs
    double *fm_again = nullptr;
    // time-tiled FM loop (qh_tiled.hpp): per tile the loop state where its warm-up and where the tile ends, and the count of
    // tiles pll_verify_kernel had to re-run
    double *pll_ends = nullptr;
    long long pll_ends_cap = 0;             // tiles per channel
    double *am_tsum = nullptr;              // [nch][am_tsum_cap][2]: the AM nbp0 tiles' contributions to the fade leveller (osfir_kernel DET 2)
    long long am_tsum_cap = 0;
    double *seg_sum[3] = { nullptr, nullptr, nullptr };     // segment summaries of the multi-workgroup scans: AM / SAM, (unused), snotch
    int *pll_nfixed = nullptr;
    // xwcpagc in time tiles (qh_agc_tiled.hpp): streams RM / fba / hba / volts per listed channel, the tiles' halos, the last samples
    // of the rows, the lanes' states, the final states, tiles re-run
    double *agc_scr = nullptr, *agc_ends = nullptr, *agc_fin = nullptr, *agc_sege = nullptr, *agc_tsum = nullptr;
    double2 *agc_halo = nullptr, *agc_tail = nullptr;
    long long agc_arr = 0, agc_ends_cap = 0, agc_halo_cap = 0;
    int *agc_nfixed = nullptr;
    // SAM sideband modes over time segments (qh_tiled.hpp, sam_sb_*): the chains' transition matrices for the two segment lengths of
    // the current call shape, the segments' zero-state end states and their start states
    double *sb_phi = nullptr, *sb_sum = nullptr, *sb_start = nullptr;
    long long sb_phi_key = -1;
    int set_sb_phi(long long n, int S);
    SamChanParam *sam_prm = nullptr;
    PllParam sam_pll_prm{}, fm_pll_prm{};
    SnotchParam *sn_prm = nullptr;
    SnotchState *sn_state = nullptr;
    // The design rows of xfmd's two filters ([0] de-emphasis, [1] audio) as they stand on the device: row r of the stage's masks holds
    // fm_rows[s][r] (key and taps; the taps are kept so that a row that only moves is uploaded, not designed, again) and channel ch reads
    // row fm_row_of[s][ch].  fm_dirty: a setter, the lists or the masks' layout moved; fm_relayout: every row is to be uploaded again.
    struct FmRow {
        int nc = 0, mp = 0; double f_low = 0.0, f_high = 0.0;
        std::vector<cd> taps;
        bool real = true;
        bool same(const FmRow &o) const { return nc == o.nc && mp == o.mp && f_low == o.f_low && f_high == o.f_high; }
    };
    std::vector<FmRow> fm_rows[2];
    std::vector<int> fm_row_of[2];
    bool fm_dirty = true, fm_relayout = false;
    int fm_key_built = 0;
    long long fm_designed = 0;              // rows designed on the host so far (diagnostics: qh_rxa_debug_fm_rows)
    // the ping-pong halves in use: bit 0 the front stage's, bit 1 + s fircore stage s's -- one captured launch sequence per value
    static_assert(sizeof(graph_slot) / sizeof(graph_slot[0]) == 1u << (1 + FC_COUNT), "one graph slot per state of the ping-pong flags");
    unsigned flags() const { unsigned f = (unsigned)cur_front; for (int s = 0; s < FC_COUNT; s++) f |= (unsigned)fc[s].cur << (1 + s); return f; }
    void set_flags(unsigned f) { cur_front = f & 1; for (int s = 0; s < FC_COUNT; s++) fc[s].cur = f >> (1 + s) & 1; }
    void drop_graphs() { for (auto &g : graph_slot) if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; } }
    // Growing, rebuilding or re-uploading a device buffer: captured launch sequences hold its address and launches queued on either
    // stream may still use it, so nothing is freed or rewritten before quiesce() has waited for both streams and dropped the captures.
    int quiesce();
    // (Re)allocate p for n elements (dev_alloc), zeroed on `stream` when asked.  A buffer p held is freed first: the caller has quiesced.
    template <typename T> int alloc(T *&p, long long n, bool zero = false);
    // give a buffer alloc() made back (the caller has quiesced)
    template <typename T> void release(T *&p) { if (p) { (void)hipFree(p); owned.erase(p); p = nullptr; } }
    // p holds cap units of `unit` elements: when need is more, quiesce and reallocate it for need units
    template <typename T> int grow(T *&p, long long &cap, long long need, long long unit);
    int process_replayed(const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk);
    AgcParam *agc_prm = nullptr;
    AgcState *agc_state = nullptr;
    // xwcpagc's ring in full (RB_SIZE entries per channel, qh_demod.hpp: agc_long_mirror_kernel), made when a state machine first runs
    double2 *agc_lring = nullptr;
    double *agc_labs = nullptr;
    int *agc_lout = nullptr, *agc_rewin_list = nullptr;
    AgcParam *lim_prm = nullptr;        // FM detector limiter: a wcpAGC of its own (fmd.c:48-72)
    AgcState *lim_state = nullptr;
    MeterState *m_adc = nullptr, *m_s = nullptr, *m_agc = nullptr;
    MeterParam m_prm{};
    // meters fused into the nbp0 launch of the linear fast path (qh_osfir.hpp METER): per tile and row of 16 lanes partials of the
    // stage's input and output, the taps' tables (lane weights and the peak's decay per block: kMeterTabDoubles), and g^2 of a
    // fixed AGC gain that the output matrix applies behind the agc meter's tap
    double2 *m_part[2] = { nullptr, nullptr };
    long long m_part_cap = 0;               // partials per channel
    double *m_w = nullptr, *m_g2 = nullptr;
    int meters_alloc();
    int meter_parts() const { return kMeterRows * (band6k ? 6 : band2g ? 8 : 4); }       // a tile's partials: one per row of 16 lanes of the band tile in use
    int agc_last_tiled = 0;             // channels whose xwcpagc took the time tiles in the last call (diagnostics)
    int n_agc_cur_stale = 0, n_agc_other_stale = 0;     // ... of which, at the lists' ends, channels whose attack window moved in mid-stream

    ~Engine();
    int init();
    // init's two rate-dependent ends, each made again on its own when its rate changes (set_rates): the front stage for in_rate / dsp_rate
    // (dsp_insize, D, the overlap-save tables and delay line or the polyphase rsmpin) and rsmpout for dsp_rate / out_rate (dsp_outsize)
    int front_build();
    int out_build();
    // The run-time setters of wdsp/channel.c:169-258 on a live engine (qh_rxa_set_rates ...): see the definition for what survives
    int set_rates(int new_in, int new_dsp, int new_out, int new_size);
    int rebuild(int new_in, int new_dsp, int new_out, int new_size, int new_D);
    // State of stages that are made on first use, read off the device by rebuild and waiting for the allocation that makes the stage
    // again (stages_alloc, snba_alloc, gen_alloc take it and empty it): anf / anr's lidx and ngamma [nch][2] (flush_anf / flush_anr leave
    // them, anf.c:135-140), snba's frame memory [nch][2 kSnbX] (xbase / xaux are create_snba's, calc_snba does not touch them,
    // snb.c:31-66) and, across a new dsp_size, gen0's phases and positions [nch] (setSize_gen only flushes the pulse, gen.c:160-163,369-373)
    struct Carry { std::vector<double> lms[2], snba_frames; std::vector<GenState> gen; } carry;
    int flush();
    // what the parameter side needs of the kernels, defined where they are launched from (qh_engine.hip): the dynamic-LDS limits of the
    // tile kernels and of emnr_kernel, and the launches of refresh_params and flush
    int tile_lds_limits();
    int emnr_lds_limit();
    void launch_nco_retune(int n);
    void launch_nco_park(int ch, int run);
    void launch_front_masks(int n);
    void launch_ssql_flush();
    int refresh_params();
    std::vector<cd> notched(const ChanCfg &c, int nc, double f_low, double f_high, double scale) const;
    int snb_mask(ChanCfg &c, int ch);
    // the layout the one-tile masks are built for: a stage's masks are made again when it moves (pick_band_tile)
    int mask_key() const { return 2 * bnfft + (band2g ? 1 : 0); }
    int fc_alloc(Fircore &f);
    int put_taps(Fircore &f, int row, const std::vector<cd> &h, std::vector<cd> &m);
    // refresh_demod and its steps
    int refresh_demod();
    int demod_init();
    void build_lists(std::vector<int> (&h)[L_COUNT]);
    int stages_alloc();
    int refresh_lists();
    int fc_follow(Fircore &f, const std::vector<int> &chans);
    int zero_rows(Fircore &f, int ch, int n = 1);
    int prm_agc(ChanCfg &c, int ch);
    int prm_emnr(ChanCfg &c, int ch);
    int prm_snba(ChanCfg &c, int ch);
    int prm_amsq(ChanCfg &c, int ch);
    int prm_lms(ChanCfg &c, int ch);
    int prm_lim(ChanCfg &c, int ch);
    int prm_detect(ChanCfg &c, int ch);
    int fm_filters();
    int fm_rows_resize(Fircore &f, int rows);
    // v -> dev[row] on `stream`, then a wait unless told not to (a caller that does not wait keeps v alive until it does)
    template <typename T> int put_row(T *dev, long long row, const T &v, bool wait = true)
    {
        QH_HIP(hipMemcpyAsync(dev + row, &v, sizeof(T), hipMemcpyHostToDevice, stream));
        if (wait) QH_HIP(hipStreamSynchronize(stream));
        return QH_OK;
    }
    int run_front(const double2 *src, long long src_stride, double2 *dst, long long dst_stride, const EpiParam *ep,
                  long long n_in, long long n_mid, const int *list = nullptr, int nlist = 0, int part = 0);
    const unsigned char *pk_src = nullptr;      // set for the duration of a qh_rxa_process_packed call
    PackedFmt pk{};
    EgressFmt eg{};                             // set (kind != 0) for the duration of a qh_rxa_process_audio call
    double2 *abuf = nullptr;                    // complex-double staging of an audio call whose last stage cannot narrow in its store
    long long abuf_cap = 0;
    int ensure_abuf(long long n);
    void pack_audio(const double2 *src, long long src_stride, long long n);
    void run_band(const double2 *src, long long src_stride, double2 *dst, long long dst_stride, const EpiParam *ep,
                  long long n_mid, Fircore &f, int P,
                  const int *list, int nlist, bool meter = false, bool egress = false, int det = 0, double *det_out = nullptr,
                  long long det_stride = 0, const int *pairs = nullptr, int npairs = 0);
    int ensure_buffers(long long n_mid);
    int ensure_meter_partials(long long n_mid, int lout);
    int emnr_alloc();
    int process(const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk);
    int process_chain(const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk);
    // One process_chain call: its sizes and rows, and the form every stage takes, each decided once where it is set below
    struct ChainCall {
        int nblk = 0, nc_max = 1, P = 0, P_am = 0;
        long long n_in = 0, n_mid = 0;
        const double2 *in = nullptr;
        long long in_stride = 0, out_stride = 0;
        double2 *out = nullptr;
        double2 *cur = nullptr, *other = nullptr;       // the mixed path's working rows (buf[0] / buf[1], swapped as stages write)
        bool any_nbp = false, any_bp1 = false, any_eqp = false, every_nbp = true, mixed = false, long_mode = false, meters_fused = false, eg_fused = false;
        bool split = false, fm_theta_fused = false, direct = false, am_fused = false, am_lv_fused = false, side = false;
        bool agc_direct = false;                        // set where xwcpagc runs (run_agc)
        bool gen = false;                               // a channel runs gen0: no two-stream split, the generating launch behind the front stage
        bool taps = false;                              // a channel runs its sender or its siphon: the stores that skip their points are off
    };
    int chain_needs(ChainCall &k);
    int plan_long(ChainCall &k);
    void pick_band_tile(int nc_max);
    int run_linear(ChainCall &k);
    int plan_mixed(ChainCall &k);
    int ensure_side_stream();
    int fork_side();
    int run_mixed_front(ChainCall &k);
    int seg_groups(int count, long long n_mid) const;
    template <bool SAM> void am_detect(const ChainCall &k, hipStream_t s, const int *list, int n, int G, const double *pts, long long pts_stride, double *gs);
    int run_am(ChainCall &k);
    int run_fm(ChainCall &k);
    void snb_inplace(const ChainCall &k, const int *list, int n);
    int run_snba(const ChainCall &k);
    void eqp_inplace(const ChainCall &k);
    void lms_at(const ChainCall &k, int pos, double2 *b);
    void bp1_at(const ChainCall &k, int pos);
    int run_agc(ChainCall &k);
    int refresh_ap(const ChainCall &k);
    void run_audio_peak(const ChainCall &k);
    int refresh_ssql(const ChainCall &k);
    void run_ssql(const ChainCall &k);
    void run_fmsq(const ChainCall &k);
    void run_sender(const ChainCall &k);
    void run_gen(const ChainCall &k);
    void run_siphon(const ChainCall &k);
    void run_output(const ChainCall &k);
    qh_rat *rsmpout = nullptr;          // xresample out (wdsp/RXA.c:596), only when out_rate != dsp_rate
    qh_rat *rsmpin = nullptr;           // xresample in for the rate ratios the overlap-save front stage does not cover (D == 0)
    double2 *fbuf = nullptr;            // its input: the shifted samples at in_rate
    long long fbuf_cap = 0;
    double2 *obuf = nullptr;
    long long obuf_cap = 0;
    void tick(int cat);
};

// What qh_rxa_create accepts (wdsp/channel.c:39-52): the status it sets, QH_OK with *D = in_rate / dsp_rate where the overlap-save front
// stage covers the ratio (1, 2, 4, 8, 16), else 0 (the polyphase form of xresample).  `who` heads the message.
int check_rates(const char *who, int dsp_size, int in_rate, int dsp_rate, int out_rate, int *D);
// whether two of an EQ profile's frequencies coincide after eq_impulse's clamp to [0, 1] (eq.c:53-55) while their gains differ
bool eqp_profile_tie(const std::vector<double> &F, const std::vector<double> &G, double rate);

// egress_pack_kernel over nch rows of n samples (Engine::pack_audio, qh_audio_pack)
void launch_egress_pack(const double2 *src, long long src_stride, int nch, long long n, const EgressFmt &f, hipStream_t s);

template <typename T> int Engine::alloc(T *&p, long long n, bool zero)
{
    if (p) { QH_HIP(hipFree(p)); owned.erase(p); p = nullptr; }
    QH_HIP(dev_alloc(&p, (size_t)n));
    owned[p] = n * (long long)sizeof(T);
    if (zero) QH_HIP(hipMemsetAsync(p, 0, (size_t)n * sizeof(T), stream));
    return QH_OK;
}

template <int R> int Engine::list_make(ListBlock<R> &b)
{
    if (int rc = alloc(b.block, (long long)R * nch)) return rc;
    for (int r = 0; r < R; r++) b.row[r].dev = b.block + (size_t)nch * r;
    return QH_OK;
}

template <int R> int Engine::list_upload(ListBlock<R> &b)
{
    if (!b.block) return QH_OK;
    b.image.assign((size_t)R * nch, 0);
    for (int r = 0; r < R; r++) std::copy(b.h[r].begin(), b.h[r].end(), b.image.begin() + (size_t)nch * r);
    QH_HIP(hipMemcpyAsync(b.block, b.image.data(), b.image.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    return QH_OK;
}

template <typename T> int Engine::grow(T *&p, long long &cap, long long need, long long unit)
{
    if (need <= cap) return QH_OK;
    if (int rc = quiesce()) return rc;
    if (int rc = alloc(p, need * unit)) return rc;
    cap = need;
    return QH_OK;
}

}  // namespace qh

// One lock per engine: setters may come from another thread than the one that runs the blocks (Quisk's GUI thread against its
// sound thread; WDSP's setters take csDSP).  A setter only edits the host-side configuration and marks it dirty; the next
// process call uploads what changed before it enqueues the block, so parameters swap on a block boundary.
struct qh_rxa { qh::Engine e; std::recursive_mutex mtx; };
#define QH_RXA_LOCK(h) std::lock_guard<std::recursive_mutex> _lk((h)->mtx)
