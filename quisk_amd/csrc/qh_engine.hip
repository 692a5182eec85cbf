// qh_engine.hip -- batched RXA receive engine for MI355X and its C ABI (include/quiskhip.h, group 1).
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
//   hist_nbp   [2][nch][HB]  nbp0 input samples  (the reference's fircore delay line)
//   hist_bp1   [2][nch][HB]
//   nco_phase  [nch]         64-bit fixed-point turns
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
#include "qh_kernels.hpp"
#include "qh_demod.hpp"
#include "qh_tiled.hpp"
#include "qh_agc_tiled.hpp"
#include "qh_emnr.hpp"
#include "qh_snba.hpp"
#include "qh_audio_peak.hpp"
#include "qh_ssql.hpp"
#include "qh_internal.hpp"

namespace qh {

thread_local std::string g_last_error;

int set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

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
    int shift_on_device = 1;                                    // whether the device phase is live or parked (nco_park_kernel)
    int nbp_run = 1, nbp_nc = 2048, nbp_wintype = 0;            // RXA.c:90-106
    int mp = 0;                                                 // RXASetMP, RXA.c:948
    // notch database (create_notchdb RXA.c:85-87) and nbp0's use of it (fnfrun 0, autoincr 1: RXA.c:92,104)
    std::vector<Notch> notches;
    double ndb_tunefreq = 0.0, ndb_shift = 0.0;
    int fnfrun = 0, autoincr = 1;
    double nbp_flow = -4150.0, nbp_fhigh = -150.0, nbp_gain = 1.0;
    int amd_run = 0, amd_mode = 0, fmd_run = 0;                 // RXA.c:175-212
    int agc_run = 1, agc_mode = 3; double agc_fixed = 1000.0;   // RXA.c:335-358
    double agc_tau_attack = 0.001, agc_tau_decay = 0.250, agc_max_gain = 10000.0, agc_var_gain = 1.5;
    double agc_hangtime = 0.250, agc_hang_thresh = 0.250;
    bool agc_dirty = true;
    bool agc_on() const { return agc_run && agc_mode != 0; }
    int agc_abuf = -1;                  // attack_buffsize last uploaded
    bool agc_rewindow = false;          // the attack window moved in mid-stream: the state's ring is taken again from the full one
    bool agc_ran = false, agc_stale = false;    // the window moved while the ring held samples: ring_max may be stale (qh_agc_tiled.hpp)
    int bp1_run = 1, bp1_nc = 2048, bp1_wintype = 1;            // RXA.c:377-389
    bool long_live[5] = { false, false, false, false, false };  // the channel holds a delay line of stage sid longer than 4095 samples (process_chain)
    double bp1_flow = -4150.0, bp1_fhigh = -150.0, bp1_gain = 1.0;
    double gain1 = 4.0, gain2I = 1.0, gain2Q = 1.0;             // RXA.c:464-474
    int inselect = 3, copy = 0;
    int levelfade = 1, sbmode = 0;                              // RXA.c:180-181
    double fm_dev = 5000.0, ctcss_freq = 254.1;                 // RXA.c:198,208
    int ctcss_run = 1, fm_nc = 2048;                            // RXA.c:207,209-212
    int lim_run = 0; double lim_gain = 2.5; bool lim_dirty = true;   // FM detector limiter, fmd.c:106-108
    // anf / anr (create_anf / create_anr of create_rxa, RXA.c:278-315): [0] = anf, [1] = anr
    struct Lms { int run = 0, position = 0, taps = 64, delay = 16; double two_mu = 0.0001, gamma = 0.1; bool dirty = true, flush = false; } lms[2];
    // emnr (create_emnr of create_rxa, RXA.c:319-332)
    // snba (wdsp/snb.c) and its bandpass bpsnba (snb.c:696-855; run / position follow the mode, RXA.c:883-917)
    int snba_run = 0, snb_hist_at = 0;
    int fm_hist_at = 0;                                         // ping-pong half that holds this channel's FM fircore delay lines
    int bp1_hist_at = 0;                                        // ... and bp1's (SetRXABandpassRun switches it on WITHOUT the flush of RXAbp1Set)
    bool snba_flush = false, snba_taps_dirty = true, snba_rout_flush = false, snb_dirty = true, snb_flush = false;
    double snba_f_low = 200.0, snba_f_high = 0.0;               // outresamp fc_low / fcin (snb.c:45-46, resample.c:195-204)
    int snb_pos() const {
        if (!snba_run) return -1;
        switch (mode) {
        case QH_LSB: case QH_CWL: case QH_DIGL: case QH_USB: case QH_CWU: case QH_DIGU: return 0;
        case QH_AM: case QH_SAM: case QH_DSB: case QH_FM: return 1;
        default: return -1;
        }
    }
    int emnr_run = 0, emnr_pos = 0, emnr_gain_method = 2, emnr_npe = 0, emnr_ae = 1; bool emnr_dirty = true, emnr_flush = false;
    double emnr_ae_zeta = 0.75, emnr_ae_psi = 20.0, emnr_train_zeta = -2.0, emnr_train_t2 = 0.20;       // emnr.c:332,491-493
    // amsq (create_amsq of create_rxa, RXA.c:158-172)
    int amsq_run = 0; double amsq_tail_thresh = 0.009, amsq_unmute_thresh = 0.010, amsq_max_tail = 1.5; bool amsq_dirty = true;
    int bp1_pos = 0;                                            // SetRXAANFPosition / SetRXAANRPosition set it too (anf.c:236)
    // xwcpagc mode 0 with a position-1 stage behind it: the gain is applied in place at the AGC's spot, not in the epilogue
    bool demod_dirty = true, ctcss_flush = false;
    bool nbp_dirty = true, bp1_dirty = true, nco_dirty = true, epi_dirty = true;
    bool nbp_flush = false, bp1_flush = false;
    // xcbl, xspeak, xmpeak (create_rxa, RXA.c:403-445: all three made with run 0); the design setters zero their cascade (sp_flush,
    // mp_flush) at the next block boundary
    int cbl_run = 0, sp_run = 0, mp_run = 0, mp_npeaks = 2;
    double sp_f = 600.0, sp_bw = 100.0, sp_gain = 2.0;
    int mp_enable[kApPeaks] = { 1, 1 };
    double mp_f[kApPeaks] = { 2125.0, 2295.0 }, mp_bw[kApPeaks] = { 75.0, 75.0 }, mp_gain[kApPeaks] = { 1.0, 1.0 };
    bool ap_dirty = true, sp_flush = false, mp_flush[kApPeaks] = { false, false };
    bool ap_on() const { return cbl_run || sp_run || mp_run; }
    // xssql (create_ssql of create_rxa, RXA.c:447-461: run 0, wthresh 0.08, tau_mute = tau_unmute = 0.1); no setter flushes it
    int ssql_run = 0;
    double ssql_wthresh = 0.08, ssql_tau_mute = 0.1, ssql_tau_unmute = 0.1;
    bool ssql_dirty = true;
    bool ssql_on() const { return ssql_run != 0; }
    // (the new stages sit behind xwcpagc too, ahead of the panel: a fixed gain that changes while a peak still rings must not reach
    // the ringing tail, so it is applied at the AGC's spot for them as well; SSQL's detector reads amplitude, so it needs the gain too)
    bool fix_before() const
    {
        return agc_run && agc_mode == 0 && ((bp1_run && bp1_pos) || (lms[0].run && lms[0].position) || (lms[1].run && lms[1].position) ||
                                            (emnr_run && emnr_pos) || ap_on() || ssql_on());
    }
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
    bool graph_on = false, graph_seen = false;
    GraphKey graph_key;
    GraphSlot graph_slot[64];
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
    double2 *mask_front = nullptr, *mask_nbp = nullptr, *mask_bp1 = nullptr;
    double2 *tw4096 = nullptr, *tw_inv_front = nullptr, *tw8192 = nullptr;
    int bnfft = kNfft;                      // tile size of the fircore stages: what their masks are built for (4096 or 8192)
    bool band2g = false;                    // 8192-point tiles shared by two lane groups (osfir8k_kernel): masks stored [even | odd]
    bool band6k = false;                    // 6144-point tiles on 384 lanes (osfir6k_kernel)
    int dbg_forms = [] { const char *e = std::getenv("QH_DBG_FORMS"); return e ? std::atoi(e) : 0; }();   // see process_chain
    int band_tile_pref = 0;                 // qh_rxa_set_band_tile: 0 / 4096: 4096-point tiles, 8192: the two-group tiles
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
    double2 *hist_front[2] = { nullptr, nullptr }, *hist_nbp[2] = { nullptr, nullptr }, *hist_bp1[2] = { nullptr, nullptr };
    int cur_front = 0, cur_nbp = 0, cur_bp1 = 0, cur_snb = 0;
    double2 *mask_snb = nullptr, *hist_snb[2] = { nullptr, nullptr };
    double2 *buf[2] = { nullptr, nullptr };
    long long buf_cap = 0;                  // complex samples per channel
    // long impulse responses (nc > 4096), per fircore stage s = 0 nbp0, 1 bp1, 2 FM de-emphasis, 3 FM audio filter, 4 bpsnba:
    // long_parts[s] partitions (1: the ordinary path), their masks lmask[s] ([nch or 1][kLongParts][8192]), how many of them each mask row's
    // own impulse response reaches lrow_parts[s] ([nch or 1]), the stage's last kLongHist input samples lhist[s][ping-pong][nch][kLongHist];
    // lcat: history + block of the stage being run, ltmp: a partition's output
    int long_parts[5] = { 1, 1, 1, 1, 1 };
    double2 *lmask[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    int *lrow_parts[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    double2 *lhist[5][2] = { { nullptr, nullptr }, { nullptr, nullptr }, { nullptr, nullptr }, { nullptr, nullptr }, { nullptr, nullptr } };
    double2 *lcat = nullptr, *ltmp = nullptr;
    long long lcat_cap = 0;                 // the buf_cap they were made for
    int long_stage_alloc(int sid, bool shared_mask);
    int long_buffers();
    int long_masks_upload(int sid, long long row, const std::vector<cd> &h);
    // Every device buffer the engine owns, by its address, and its size in bytes: alloc() enters it, ~Engine frees it, dev_bytes()
    // adds them up (the qh_rat resamplers hold their own)
    std::map<void *, long long> owned;
    long long dev_bytes() const { long long b = 0; for (const auto &o : owned) b += o.second; return b; }
    // timing
    bool timing = false;
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
    int *list_block = nullptr;
    // channel pairs for the real filters behind the detectors (osfir_kernel PAIR): FM de-emphasis (one mask for all), bp1 of the AM
    // and of the SAM channels (partners have the same design; count 0 when a channel of the kind has complex taps)
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
    // xssql (qh_ssql.hpp), made when a channel first runs it: its two channel lists (by the buffer that holds the row, as L_AP; a
    // block of their own, so that an engine without SSQL allocates what it did before), parameters, state, the ramps, the tiles' rows
    // [nch][ssql_ends_cap][kSsE], the crossing / window / trigger bits [3][nch][ssql_wcap] and the words' machine records [nch][ssql_wcap]
    ChanList ssql_lists[2];
    std::vector<int> ssql_h[2];
    int *ssql_list_block = nullptr;
    SsqlParam *ssql_prm = nullptr;
    SsqlState *ssql_state = nullptr;
    double *ssql_cup = nullptr, *ssql_cdown = nullptr, *ssql_ends = nullptr;
    unsigned long long *ssql_bits = nullptr;
    int *ssql_rec = nullptr;
    long long ssql_ends_cap = 0, ssql_wcap = 0, ssql_rec_cap = 0;
    int ssql_L = 0, ssql_ntup = 0, ssql_ntdown = 0;
    std::vector<SsqlParam> ssql_prm_h;
    int ssql_alloc();
    bool ssql_listed() const { return ssql_lists[0].n || ssql_lists[1].n; }
    // snba: the blanker's parameters, taps, state and the Toeplitz-inverse scratch
    SnbaParam snba_prm{};
    double *snba_state = nullptr, *snba_hin = nullptr, *snba_hout = nullptr, *snba_scratch = nullptr;
    SnbaIdx *snba_idx = nullptr;
    SnbaTune *snba_tune = nullptr;          // [nch]; host copy below, uploaded when a tuning setter has run
    std::vector<SnbaTune> snba_tune_h;
    bool snba_tune_dirty = true;
    std::vector<char> snb_listed, fm_listed, bp1_listed;
    int snba_alloc();
    int snba_ovrlp = 4;                 // create_rxa's overlap (RXA.c:244): incr = xsize / 4
    void snba_plan(int ovrlp);
    int snba_set_ovrlp(int ovrlp);
    EmnrParam emnr_prm{};
    EmnrChan *emnr_chan = nullptr;
    EmnrScalars *emnr_scal = nullptr;
    double *emnr_state = nullptr, *emnr_window = nullptr, *emnr_GG = nullptr, *emnr_GGS = nullptr, *emnr_zeta = nullptr;
    int *emnr_zeta_true = nullptr;
    bool emnr_tables = false;
    std::vector<double> h_GG, h_GGS, h_zeta; std::vector<int> h_zeta_true; double h_zrange[4] = { 0, 0, 0, 0 };
    AmsqParam *amsq_prm = nullptr;
    AmsqState *amsq_state = nullptr;
    double *amsq_cup = nullptr, *amsq_cdown = nullptr, *amsq_mag = nullptr;
    long long amsq_mag_cap = 0;
    int amsq_ntup = 0, amsq_ntdown = 0;
    LmsParam *lms_prm[2] = { nullptr, nullptr };
    LmsState *lms_state[2] = { nullptr, nullptr };
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
    int pll_check_only = 0;                 // diagnostics (qh_rxa_debug_pll): count unconverged tiles without re-running them
    int agc_form = 0;                       // diagnostics (qh_rxa_debug_agc): 1 = the sample-by-sample form of the wcpAGC loop
    SamChanParam *sam_prm = nullptr;
    PllParam sam_pll_prm{}, fm_pll_prm{};
    SnotchParam *sn_prm = nullptr;
    SnotchState *sn_state = nullptr;
    double2 *mask_de = nullptr, *mask_aud = nullptr, *hist_de[2] = { nullptr, nullptr }, *hist_aud[2] = { nullptr, nullptr };
    int cur_de = 0, cur_aud = 0, fm_nc_built = 0, fm_mp = 0, fm_mp_built = 0, fm_nfft_built = 0;
    unsigned flags() const { return (unsigned)(cur_front | cur_nbp << 1 | cur_bp1 << 2 | cur_de << 3 | cur_aud << 4 | cur_snb << 5); }
    void set_flags(unsigned f) { cur_front = f & 1; cur_nbp = f >> 1 & 1; cur_bp1 = f >> 2 & 1; cur_de = f >> 3 & 1; cur_aud = f >> 4 & 1; cur_snb = f >> 5 & 1; }
    void drop_graphs() { for (auto &g : graph_slot) if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; } }
    // Growing, rebuilding or re-uploading a device buffer: captured launch sequences hold its address and launches queued on either
    // stream may still use it, so nothing is freed or rewritten before quiesce() has waited for both streams and dropped the captures.
    int quiesce();
    // (Re)allocate p for n elements (dev_alloc), zeroed on `stream` when asked.  A buffer p held is freed first: the caller has quiesced.
    template <typename T> int alloc(T *&p, long long n, bool zero = false);
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
    bool meters_on = false;
    MeterState *m_adc = nullptr, *m_s = nullptr, *m_agc = nullptr;
    MeterParam m_prm{};
    // meters fused into the nbp0 launch of the linear fast path (qh_osfir.hpp METER): chunk partials of the stage's input and
    // output, the chunk weights, and g^2 of a fixed AGC gain that the output matrix applies behind the agc meter's tap
    double2 *m_part[2] = { nullptr, nullptr };
    long long m_part_cap = 0;               // chunks per channel
    double *m_w = nullptr, *m_g2 = nullptr;
    int meters_alloc();
    int agc_last_tiled = 0;             // channels whose xwcpagc took the time tiles in the last call (diagnostics)
    int n_agc_cur_stale = 0, n_agc_other_stale = 0;     // ... of which, at the lists' ends, channels whose attack window moved in mid-stream

    ~Engine();
    int init();
    int refresh_params();
    std::vector<cd> notched(const ChanCfg &c, double f_low, double f_high, double scale) const;
    int snb_mask(ChanCfg &c, int ch);
    int put_mask(double2 *mask, int ch, const std::vector<cd> &m);
    // refresh_demod and its steps
    int refresh_demod();
    int demod_init();
    void build_lists(std::vector<int> (&h)[L_COUNT]);
    int stages_alloc();
    int refresh_lists();
    struct Rows { double2 **h; int cur; int len; };     // a fircore's ping-pong delay lines, the half current for them, the row length
    int follow_rows(std::vector<char> &listed, int ChanCfg::*at, int cur, const std::vector<int> &chans, std::initializer_list<Rows> rows);
    int zero_rows(double2 *const h[2], double2 *const lh[2], int ch, int n = 1);
    int prm_agc(ChanCfg &c, int ch);
    int prm_emnr(ChanCfg &c, int ch);
    int prm_snba(ChanCfg &c, int ch);
    int prm_amsq(ChanCfg &c, int ch);
    int prm_lms(ChanCfg &c, int ch);
    int prm_lim(ChanCfg &c, int ch);
    int prm_detect(ChanCfg &c, int ch);
    int fm_filters(int want_nc);
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
                  long long n_mid, const double2 *mask, long long mask_stride, double2 **hist, int &hc, int P,
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
        bool any_nbp = false, any_bp1 = false, every_nbp = true, mixed = false, long_mode = false, meters_fused = false, eg_fused = false;
        bool split = false, fm_theta_fused = false, direct = false, am_fused = false, am_lv_fused = false, side = false;
        bool agc_direct = false;                        // set where xwcpagc runs (run_agc)
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
    void lms_at(const ChainCall &k, int pos, double2 *b);
    void bp1_at(const ChainCall &k, int pos);
    int run_agc(ChainCall &k);
    int refresh_ap(const ChainCall &k);
    void run_audio_peak(const ChainCall &k);
    int refresh_ssql(const ChainCall &k);
    void run_ssql(const ChainCall &k);
    void run_output(const ChainCall &k);
    qh_rat *rsmpout = nullptr;          // xresample out (wdsp/RXA.c:596), only when out_rate != dsp_rate
    qh_rat *rsmpin = nullptr;           // xresample in for the rate ratios the overlap-save front stage does not cover (D == 0)
    double2 *fbuf = nullptr;            // its input: the shifted samples at in_rate
    long long fbuf_cap = 0;
    double2 *obuf = nullptr;
    long long obuf_cap = 0;
    void tick(int cat);
};

Engine::~Engine()
{
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    drop_graphs();
    if (rsmpout) qh_rat_destroy(rsmpout);
    if (rsmpin) qh_rat_destroy(rsmpin);
    for (const auto &o : owned) (void)hipFree(o.first);
    for (auto e : ev) (void)hipEventDestroy(e);
    if (side_stream) (void)hipStreamDestroy(side_stream);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

static int upload(double2 *dst, const std::vector<cd> &v, hipStream_t s)
{
    QH_HIP(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(cd), hipMemcpyHostToDevice, s));
    QH_HIP(hipStreamSynchronize(s));        // the host vector dies with the caller's scope
    return QH_OK;
}

int Engine::quiesce()
{
    QH_HIP(hipStreamSynchronize(stream));
    if (side_stream) QH_HIP(hipStreamSynchronize(side_stream));
    drop_graphs(); epoch++;
    return QH_OK;
}

template <typename T> int Engine::alloc(T *&p, long long n, bool zero)
{
    if (p) { QH_HIP(hipFree(p)); owned.erase(p); p = nullptr; }
    QH_HIP(dev_alloc(&p, (size_t)n));
    owned[p] = n * (long long)sizeof(T);
    if (zero) QH_HIP(hipMemsetAsync(p, 0, (size_t)n * sizeof(T), stream));
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

int Engine::init()
{
    QH_HIP(hipSetDevice(device));
    if (!stream) { QH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); own_stream = true; }
    // pre_main_build, wdsp/channel.c:39-47
    dsp_insize = D > 0 ? dsp_size * D : (int)((long long)dsp_size * in_rate / dsp_rate);
    if (D == 0) {
        // create_resample(..., in_rate, dsp_rate, 0.0, 0, 1.0), wdsp/RXA.c:48-57
        const ResamplerDesign rd = design_resampler(in_rate, dsp_rate, 0.0, 0, 1.0);
        std::vector<double> taps(rd.h);
        for (double &v : taps) v /= (double)rd.L;           // qh_rat applies the gain `interp` itself (quisk_cInterpDecim's convention)
        rsmpin = qh_rat_create(device, nch, taps.data(), rd.ncoef, rd.L, rd.M, QH_F64, stream);
        if (!rsmpin) return QH_ERR_HIP;
    }
    dsp_outsize = out_rate >= dsp_rate ? dsp_size * (out_rate / dsp_rate) : dsp_size / (dsp_rate / out_rate);    // channel.c:47-50
    if (out_rate != dsp_rate) {
        // create_resample(..., dsp_rate, out_rate, 0.0, 0, 1.0), wdsp/RXA.c:474-484; the polyphase loop of xresample
        // (resample.c:120-157) is quisk_cInterpDecim's with the gain already in the taps
        const ResamplerDesign rd = design_resampler(dsp_rate, out_rate, 0.0, 0, 1.0);
        std::vector<double> taps(rd.h);
        for (double &v : taps) v /= (double)rd.L;
        rsmpout = qh_rat_create(device, nch, taps.data(), rd.ncoef, rd.L, rd.M, QH_F64, stream);
        if (!rsmpout) return QH_ERR_HIP;
    }
    cfg.assign((size_t)nch, ChanCfg());
    snba_tune_h.assign((size_t)nch, SnbaTune{ 64, 2, 10, 2, 2, 0, 8.0, 20.0, 0.5 });         // create_snba's arguments, RXA.c:183-202

    std::vector<cd> tw = fft_twiddle_table(kNfft);
    if (int rc = alloc(tw4096, (long long)tw.size())) return rc;
    if (int rc = upload(tw4096, tw, stream)) return rc;
    tw = fft_twiddle_table(kBandNfftMax);
    if (int rc = alloc(tw8192, (long long)tw.size())) return rc;
    if (int rc = upload(tw8192, tw, stream)) return rc;

    if (D > 1) {
        // calc_resample, wdsp/resample.c:35-72 (L = 1): y[m] = sum_j h[j] x[D*m - j]
        ResamplerDesign rd = design_resampler(in_rate, dsp_rate, 0.0, 0, 1.0);
        if (rd.L != 1 || rd.M != D) return set_error(QH_ERR_UNSUPPORTED, "resampler L/M = %d/%d not supported", rd.L, rd.M);
        front_ntaps = rd.ncoef;
        // spectral fold by min(D, 8); the rest of the decimation (D = 16) keeps every second folded sample
        front_fold = D > 8 ? 8 : D;
        front_pick = D / front_fold;
        front_P = ((front_ntaps - 1 + front_fold - 1) / front_fold) * front_fold;
        front_L = (((kNfft - front_P) / front_fold) / front_pick) * front_pick;
        if (front_P > kHistFront) return set_error(QH_ERR_UNSUPPORTED, "resampler history %d too long", front_P);
        // the masks are per channel (taps modulated by the channel's shift): front_mask_kernel builds them in refresh_params
        if (int rc = alloc(mask_front, (long long)nch * kNfft)) return rc;
        if (int rc = alloc(lane_rot, (long long)nch * NT)) return rc;
        if (int rc = alloc(front_taps, front_ntaps)) return rc;
        if (int rc = alloc(retune_list, nch)) return rc;
        if (int rc = alloc(retune_law, 2LL * nch)) return rc;
        QH_HIP(hipMemcpyAsync(front_taps, rd.h.data(), (size_t)front_ntaps * sizeof(double), hipMemcpyHostToDevice, stream));
        QH_HIP(hipStreamSynchronize(stream));
        QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&front_mask_kernel<kNfft>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (TileFft<kNfft, false, double2>::kLdsBytes)));
        std::vector<cd> twi = fft_twiddle_table(kNfft / front_fold);
        if (int rc = alloc(tw_inv_front, (long long)twi.size())) return rc;
        if (int rc = upload(tw_inv_front, twi, stream)) return rc;
        for (double2 *&h : hist_front) if (int rc = alloc(h, (long long)nch * kHistFront, true)) return rc;
    }
    if (int rc = alloc(mask_nbp, (long long)nch * kBandNfftMax)) return rc;
    if (int rc = alloc(mask_bp1, (long long)nch * kBandNfftMax)) return rc;
    for (int i = 0; i < 2; i++) {
        if (int rc = alloc(hist_nbp[i], (long long)nch * kHistBand, true)) return rc;
        if (int rc = alloc(hist_bp1[i], (long long)nch * kHistBand, true)) return rc;
    }
    if (int rc = alloc(nco_phase, nch, true)) return rc;
    if (int rc = alloc(nco_dphase, nch, true)) return rc;
    if (int rc = alloc(nco_parked, nch, true)) return rc;
    if (int rc = alloc(nco_step, nch)) return rc;
    if (int rc = alloc(epi, nch)) return rc;

    // dynamic LDS of the overlap-save kernels
#define QH_SET_LDS(D, ...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir_kernel<double, 4096, D, __VA_ARGS__>), \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (osfir_lds_bytes<double, 4096, D, true>())))
    QH_SET_LDS(1, false); QH_SET_LDS(1, false, false, true);
    QH_SET_LDS(1, false, false, false, false, true); QH_SET_LDS(1, false, false, true, false, true);
#define QH_SET_LDS8(...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir_kernel<double, kBandNfftMax, 1, false, false, __VA_ARGS__>), \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (osfir_lds_bytes<double, kBandNfftMax, 1, true>())))
    QH_SET_LDS8(false, false, false); QH_SET_LDS8(true, false, false); QH_SET_LDS8(false, false, true); QH_SET_LDS8(true, false, true);
#undef QH_SET_LDS8
#define QH_SET_LDS6K(...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir6k_kernel<__VA_ARGS__>), \
        hipFuncAttributeMaxDynamicSharedMemorySize, osfir6k_lds_bytes()))
    QH_SET_LDS6K(false, false); QH_SET_LDS6K(true, false); QH_SET_LDS6K(false, true); QH_SET_LDS6K(true, true);
#undef QH_SET_LDS6K
#define QH_SET_LDS2G(...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir8k_kernel<__VA_ARGS__>), \
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, osfir8k_lds_bytes()))
    QH_SET_LDS2G(false, false); QH_SET_LDS2G(true, false); QH_SET_LDS2G(false, true); QH_SET_LDS2G(true, true);
#undef QH_SET_LDS2G
    QH_SET_LDS(2, false, false, false, true, false, true); QH_SET_LDS(4, false, false, false, true, false, true); QH_SET_LDS(8, false, false, false, true, false, true);
    QH_SET_LDS(2, false, true, false, true, false, true); QH_SET_LDS(4, false, true, false, true, false, true); QH_SET_LDS(8, false, true, false, true, false, true);
#undef QH_SET_LDS
    QH_HIP(hipStreamSynchronize(stream));
    return QH_OK;
}

// fixed-point turns for a frequency ratio f / rate
static unsigned long long turns_fx(double f, double rate)
{
    long double t = (long double)f / (long double)rate;
    t -= floorl(t);
    long double s = t * 18446744073709551616.0L;
    if (s >= 18446744073709551616.0L) s = 0;
    return (unsigned long long)s;
}

int Engine::refresh_params()
{
    // one pass over the channels; upload only what changed
    std::vector<cd> last_nbp, last_bp1, last_nbp_h, last_bp1_h;      // masks and impulse responses of the last design made
    const ChanCfg *last_nbp_cfg = nullptr, *last_bp1_cfg = nullptr;
    // Oscillator changes (SetRXAShiftFreq / SetRXAShiftRun).  With a front FIR stage (D > 1) the oscillator sits behind
    // the filter: first the stored raw history of every changed channel is re-expressed for its new phase law (the kernel
    // reads the old law from the device arrays, so it goes first), then the arrays are updated, then the channel's
    // modulated mask and phasor tables are rebuilt.
    std::vector<int> nco_list;
    if (D > 1) {
        std::vector<unsigned long long> law;
        for (int ch = 0; ch < nch; ch++) {
            const ChanCfg &c = cfg[(size_t)ch];
            if (!c.nco_dirty) continue;
            nco_list.push_back(ch);
            const bool flip = (c.shift_run != 0) != (c.shift_on_device != 0);
            law.push_back(flip ? (c.shift_run ? 2ull : 1ull) : 0ull);
            law.push_back(c.shift_run ? turns_fx(c.shift_freq, (double)in_rate) : 0ull);
        }
        if (!nco_list.empty()) {
            QH_HIP(hipMemcpyAsync(retune_list, nco_list.data(), nco_list.size() * sizeof(int), hipMemcpyHostToDevice, stream));
            QH_HIP(hipMemcpyAsync(retune_law, law.data(), law.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(nco_retune_hist_kernel, dim3((kHistFront + NT - 1) / NT, (unsigned)nco_list.size()), dim3(NT), 0, stream,
                               hist_front[cur_front], kHistFront, nco_phase, nco_dphase, nco_parked, (const int *)retune_list,
                               (const unsigned long long *)retune_law);
            QH_HIP(hipStreamSynchronize(stream));           // the host vectors die with this scope
        }
    }
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (c.nco_dirty) {
            if ((c.shift_run != 0) != (c.shift_on_device != 0)) {
                hipLaunchKernelGGL(nco_park_kernel, dim3(1), dim3(1), 0, stream, nco_phase, nco_parked, ch, c.shift_run ? 1 : 0);
                c.shift_on_device = c.shift_run ? 1 : 0;
            }
            // calc_shift, wdsp/shift.c:29-34: delta = 2*pi*shift/rate per input sample
            if (int rc = put_row(nco_dphase, ch, c.shift_run ? turns_fx(c.shift_freq, (double)in_rate) : 0ull)) return rc;
            c.nco_dirty = false;
        }
        if (c.epi_dirty) {
            // xwcpagc mode 0 (wcpAGC.c:167-175) then xpanel (patchpanel.c:55-101) as one 2x2 real matrix
            // (with a position-1 anf / anr / bp1 behind it the gain is applied at the AGC's own spot instead: fix_before)
            const double g = (c.agc_run && c.agc_mode == 0 && !c.fix_before()) ? c.agc_fixed : 1.0;
            const double g2 = g * g;            // the agc meter reads |g z|^2 off the signal ahead of the output matrix
            if (m_g2) if (int rc = put_row(m_g2, ch, g2, false)) return rc;
            if (fix_gain) if (int rc = put_row(fix_gain, ch, c.agc_fixed, false)) return rc;
            const double gI = c.gain1 * c.gain2I, gQ = c.gain1 * c.gain2Q;
            const double sI = (double)(c.inselect >> 1), sQ = (double)(c.inselect & 1);
            EpiParam e;
            switch (c.copy) {
            default:
            case 0: e.a = gI * sI * g; e.b = 0; e.c = 0; e.d = gQ * sQ * g; break;
            case 1: e.a = gI * sI * g; e.b = 0; e.c = gQ * sI * g; e.d = 0; break;
            case 2: e.a = 0; e.b = gI * sQ * g; e.c = 0; e.d = gQ * sQ * g; break;
            case 3: e.a = 0; e.b = gI * sQ * g; e.c = gQ * sI * g; e.d = 0; break;
            }
            if (int rc = put_row(epi, ch, e)) return rc;
            c.epi_dirty = false;
        }
        if (c.nbp_dirty) c.snb_dirty = true;        // bpsnba's nbp shares nc, window, auto-increase, mp and the notch database with nbp0
        if (c.snb_dirty && c.snba_run && mask_snb) if (int rc = snb_mask(c, ch)) return rc;
        if (c.snb_flush && hist_snb[0]) if (int rc = zero_rows(hist_snb, lhist[4], ch)) return rc;         // setNc_fircore zeroes the delay line
        c.snb_flush = false;
        if (c.nbp_dirty) {
            // calc_nbp_impulse without notches, wdsp/nbp.c:234-238; identity when the filter is off
            bool same = !c.fnfrun && last_nbp_cfg && !last_nbp_cfg->fnfrun && last_nbp_cfg->nbp_run == c.nbp_run && last_nbp_cfg->nbp_nc == c.nbp_nc &&
                        last_nbp_cfg->nbp_wintype == c.nbp_wintype && last_nbp_cfg->nbp_flow == c.nbp_flow &&
                        last_nbp_cfg->nbp_fhigh == c.nbp_fhigh && last_nbp_cfg->nbp_gain == c.nbp_gain && last_nbp_cfg->mp == c.mp;
            if (!same) {
                std::vector<cd> h;
                if (c.nbp_run && c.fnfrun)
                    h = notched(c, c.nbp_flow, c.nbp_fhigh, c.nbp_gain / (double)(2 * dsp_size));
                else if (c.nbp_run)
                    h = fir_bandpass(c.nbp_nc, c.nbp_flow, c.nbp_fhigh, (double)dsp_rate, c.nbp_wintype, 1,
                                     c.nbp_gain / (double)(2 * dsp_size));
                else
                    h.assign(1, cd(1.0, 0.0));
                if (c.nbp_run && c.mp) h = mp_imp(h, 16, 0);            // calc_fircore, wdsp/firmin.c:327-328
                // the reference's unnormalised inverse FFT of 2*size points restores the 1/(2*size)
                if (c.nbp_run) for (auto &v : h) v *= (double)(2 * dsp_size);
                last_nbp_h = h;
                if ((int)h.size() > kLongPart) h.resize((size_t)kLongPart);      // (the one-tile mask is not used then)
                last_nbp = band_mask(h);
                last_nbp_cfg = &c;
            }
            if (long_parts[0] > 1) if (int rc = long_masks_upload(0, ch, last_nbp_h)) return rc;
            if (int rc = put_mask(mask_nbp, ch, last_nbp)) return rc;
            c.nbp_dirty = false;
        }
        if (c.bp1_dirty) {
            bool same = last_bp1_cfg && last_bp1_cfg->bp1_run == c.bp1_run && last_bp1_cfg->bp1_nc == c.bp1_nc &&
                        last_bp1_cfg->bp1_wintype == c.bp1_wintype && last_bp1_cfg->bp1_flow == c.bp1_flow &&
                        last_bp1_cfg->bp1_fhigh == c.bp1_fhigh && last_bp1_cfg->bp1_gain == c.bp1_gain && last_bp1_cfg->mp == c.mp;
            if (!same) {
                std::vector<cd> h;
                if (c.bp1_run) {
                    h = fir_bandpass(c.bp1_nc, c.bp1_flow, c.bp1_fhigh, (double)dsp_rate, c.bp1_wintype, 1,
                                     c.bp1_gain / (double)(2 * dsp_size));     // wdsp/bandpass.c:302
                    if (c.mp) h = mp_imp(h, 16, 0);
                    for (auto &v : h) v *= (double)(2 * dsp_size);
                } else {
                    h.assign(1, cd(1.0, 0.0));
                }
                last_bp1_h = h;
                if ((int)h.size() > kLongPart) h.resize((size_t)kLongPart);
                last_bp1 = band_mask(h);
                last_bp1_cfg = &c;
            }
            if (long_parts[1] > 1) if (int rc = long_masks_upload(1, ch, last_bp1_h)) return rc;
            if (int rc = put_mask(mask_bp1, ch, last_bp1)) return rc;
            c.bp1_dirty = false;
            lists_dirty = true;             // the channel pairs of the real bp1 filters follow the designs
        }
        if (c.nbp_flush) {      // setNc_fircore re-plans and so zeroes the delay line
            if (int rc = zero_rows(hist_nbp, lhist[0], ch)) return rc;
            c.nbp_flush = false;
        }
        if (c.bp1_flush) {      // flush_bandpass on off->on (RXA.c:825) and setNc_fircore
            if (int rc = zero_rows(hist_bp1, lhist[1], ch)) return rc;
            c.bp1_flush = false;
        }
    }
    if (!nco_list.empty())      // retune_list still holds the channels; the new dphase values are in place
        hipLaunchKernelGGL((front_mask_kernel<kNfft>), dim3((unsigned)nco_list.size()), dim3(NT), (size_t)(TileFft<kNfft, false, double2>::kLdsBytes),
                           stream, (const double *)front_taps, front_ntaps, (const unsigned long long *)nco_dphase, (const int *)retune_list, front_fold,
                           (const double2 *)tw4096, mask_front, lane_rot, nco_step, 1);
    return QH_OK;
}

// calc_nbp_impulse with the notches, wdsp/nbp.c:221-232: bands in absolute frequency, filter in baseband
std::vector<cd> Engine::notched(const ChanCfg &c, double f_low, double f_high, double scale) const
{
    const double offset = c.ndb_tunefreq + c.ndb_shift;
    const double minwidth = (c.nbp_wintype == 1 ? 2200.0 : 1600.0) / (c.nbp_nc / 256) * ((double)dsp_rate / 48000);
    std::vector<std::pair<double, double>> bands = make_nbp(c.notches, minwidth, c.autoincr, f_low + offset, f_high + offset, nullptr);
    for (auto &b : bands) { b.first -= offset; b.second -= offset; }
    return fir_mbandpass(c.nbp_nc, bands, (double)dsp_rate, scale, c.nbp_wintype);
}

// recalc_bpsnba_filter (snb.c:807-822) with RXAbpsnbaCheck's frequencies (RXA.c:829-881): 250..5700 Hz on the mode's side
int Engine::snb_mask(ChanCfg &c, int ch)
{
    double f_low = 0.0, f_high = 0.0;
    int run_notches = 0;
    switch (c.mode) {
    case QH_LSB: case QH_CWL: case QH_DIGL: f_low = -5700.0; f_high = -250.0; run_notches = c.fnfrun; break;
    case QH_USB: case QH_CWU: case QH_DIGU: f_low = 250.0; f_high = 5700.0; run_notches = c.fnfrun; break;
    case QH_AM: case QH_SAM: case QH_DSB: case QH_FM: f_low = 250.0; f_high = 5700.0; break;
    default: break;
    }
    const double scale = 1.0 / (double)(2 * dsp_size);
    if (long_parts[4] > 1) if (int rc = long_stage_alloc(4, false)) return rc;
    std::vector<cd> h = run_notches ? notched(c, f_low, f_high, scale) : fir_bandpass(c.nbp_nc, f_low, f_high, (double)dsp_rate, c.nbp_wintype, 1, scale);
    if (c.mp) h = mp_imp(h, 16, 0);
    for (auto &v : h) v *= (double)(2 * dsp_size);
    if (long_parts[4] > 1) if (int rc = long_masks_upload(4, ch, h)) return rc;
    if ((int)h.size() > kLongPart) h.resize((size_t)kLongPart);      // (the one-tile mask is not used then)
    if (int rc = put_mask(mask_snb, ch, band_mask(h))) return rc;
    c.snb_dirty = false;
    return QH_OK;
}

// a channel's row of a fircore stage's masks (the bnfft bins of the tile in use)
int Engine::put_mask(double2 *mask, int ch, const std::vector<cd> &m)
{
    QH_HIP(hipMemcpyAsync(mask + (size_t)ch * kBandNfftMax, m.data(), (size_t)bnfft * sizeof(cd), hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));
    return QH_OK;
}

// create_meter x3 (RXA.c:69-82,142-155,361-374): tau 0.1 s for average and peak decay; flush_meter -> -400 dB
int Engine::meters_alloc()
{
    if (m_adc) return QH_OK;
    const double rate = (double)dsp_rate;
    std::vector<MeterState> init((size_t)nch, MeterState{ 0.0, 0.0, -400.0, -400.0 });
    for (MeterState **pm : { &m_adc, &m_s, &m_agc }) {
        if (int rc = alloc(*pm, nch)) return rc;
        QH_HIP(hipMemcpyAsync(*pm, init.data(), (size_t)nch * sizeof(MeterState), hipMemcpyHostToDevice, stream));
    }
    m_prm.mult_average = std::exp(-1.0 / (rate * 0.100));
    m_prm.mult_peak = std::exp(-1.0 / (rate * 0.100));
    std::vector<double> w(64), g2((size_t)nch);
    for (int i = 0; i < 64; i++) w[(size_t)i] = (1.0 - m_prm.mult_average) * std::pow(m_prm.mult_average, (double)(63 - i));
    for (int ch = 0; ch < nch; ch++) {
        const ChanCfg &c = cfg[(size_t)ch];
        g2[(size_t)ch] = (c.agc_run && c.agc_mode == 0 && !c.fix_before()) ? c.agc_fixed * c.agc_fixed : 1.0;
    }
    if (int rc = alloc(m_w, 64)) return rc;
    if (int rc = alloc(m_g2, nch)) return rc;
    QH_HIP(hipMemcpyAsync(m_w, w.data(), 64 * sizeof(double), hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(m_g2, g2.data(), g2.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));
    return QH_OK;
}

// The one-time part of refresh_demod: the demodulators' state and the loop constants of the AM / SAM and FM detectors
int Engine::demod_init()
{
    const double rate = (double)dsp_rate;
    if (int rc = alloc(list_block, (long long)nch * (L_COUNT + 3))) return rc;      // the three pair lists (last) take two rows each
    for (int i = 0; i < L_COUNT; i++) lists[i].dev = list_block + (size_t)nch * (i <= L_PAIRS_FM ? i : 2 * i - L_PAIRS_FM);
    if (int rc = alloc(fix_gain, nch)) return rc;
    if (int rc = meters_alloc()) return rc;
    if (int rc = alloc(agc_prm, nch)) return rc;
    if (int rc = alloc(agc_state, nch, true)) return rc;
    const int oi = kAgcRing - 1;                        // out_index = -1 (calc_wcpagc, wcpAGC.c:34)
    for (int c = 0; c < nch; c++) if (int rc = put_row(&agc_state[c].out_index, 0, oi, false)) return rc;
    QH_HIP(hipStreamSynchronize(stream));
    if (int rc = alloc(levelfade, nch)) return rc;
    if (int rc = alloc(am_state, nch, true)) return rc;
    if (int rc = alloc(am_next, nch)) return rc;
    if (int rc = alloc(sn_next, nch)) return rc;
    if (int rc = alloc(fmdc_next, nch)) return rc;
    if (int rc = alloc(pll_state, nch, true)) return rc;
    if (int rc = alloc(fm_pll_state, nch, true)) return rc;
    if (int rc = alloc(fm_again, nch)) return rc;
    if (int rc = alloc(pll_nfixed, 1, true)) return rc;
    if (int rc = alloc(sam_prm, nch)) return rc;
    if (int rc = alloc(sn_prm, nch)) return rc;
    if (int rc = alloc(sn_state, nch, true)) return rc;
    if (int rc = alloc(mask_de, kBandNfftMax)) return rc;
    if (int rc = alloc(mask_aud, kBandNfftMax)) return rc;
    for (int i = 0; i < 2; i++) {
        if (int rc = alloc(hist_de[i], (long long)nch * kHistBand, true)) return rc;
        if (int rc = alloc(hist_aud[i], (long long)nch * kHistBand, true)) return rc;
    }
    // init_amd (wdsp/amd.c:72-89) with create_rxa's constants (RXA.c:183-189)
    {
        const double zeta = 1.0, omegaN = 250.0, tauR = 0.02, tauI = 1.4;
        PllParam &q = sam_pll_prm;
        q.omega_min = kTwoPiRef * -2000.0 / rate; q.omega_max = kTwoPiRef * 2000.0 / rate;
        q.g1 = 1.0 - std::exp(-2.0 * omegaN * zeta / rate);
        q.g2 = -q.g1 + 2.0 * (1 - std::exp(-omegaN * zeta / rate) * std::cos(omegaN / rate * std::sqrt(1.0 - zeta * zeta)));
        q.mtauR = std::exp(-1.0 / (rate * tauR)); q.onem_mtauR = 1.0 - q.mtauR;
        q.mtauI = std::exp(-1.0 / (rate * tauI)); q.onem_mtauI = 1.0 - q.mtauI;
        am_prm.mtauR = q.mtauR; am_prm.onem_mtauR = q.onem_mtauR; am_prm.mtauI = q.mtauI; am_prm.onem_mtauI = q.onem_mtauI;
        std::vector<double> pw(2 * 2048);           // mtauR^(k + 1), mtauI^(k + 1): the carried averages' weights at sample k of a 2048-sample tile
        for (int k = 0; k < 2048; k++) { pw[(size_t)k] = std::pow(q.mtauR, (double)(k + 1)); pw[(size_t)(2048 + k)] = std::pow(q.mtauI, (double)(k + 1)); }
        // ... and the lanes' scan weights of the two averages (qh_wave.hpp PoleScan: pa = m^((lane & 15) + 1), pb = m^((lane & 31) + 1), pw = m^(lane + 1))
        pw.resize(2 * 2048 + 6 * 64);
        for (int f = 0; f < 2; f++) {
            const double m = f ? q.mtauI : q.mtauR;
            for (int l = 0; l < 64; l++) {
                pw[(size_t)(2 * 2048 + (3 * f + 0) * 64 + l)] = std::pow(m, (double)((l & 15) + 1));
                pw[(size_t)(2 * 2048 + (3 * f + 1) * 64 + l)] = std::pow(m, (double)((l & 31) + 1));
                pw[(size_t)(2 * 2048 + (3 * f + 2) * 64 + l)] = std::pow(m, (double)(l + 1));
            }
        }
        if (int rc = alloc(am_pw, (long long)pw.size())) return rc;
        if (int rc = alloc(am_last, 2LL * nch, true)) return rc;
        QH_HIP(hipMemcpyAsync(am_pw, pw.data(), pw.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        QH_HIP(hipStreamSynchronize(stream));
    }
    // calc_fmd (wdsp/fmd.c:29-44) with create_rxa's constants (RXA.c:199-204)
    {
        const double zeta = 1.0, omegaN = 20000.0, tau = 0.02;
        PllParam &q = fm_pll_prm;
        q.omega_min = kTwoPiRef * -8000.0 / rate; q.omega_max = kTwoPiRef * 8000.0 / rate;
        q.g1 = 1.0 - std::exp(-2.0 * omegaN * zeta / rate);
        q.g2 = -q.g1 + 2.0 * (1 - std::exp(-omegaN * zeta / rate) * std::cos(omegaN / rate * std::sqrt(1.0 - zeta * zeta)));
        q.mtau = std::exp(-1.0 / (rate * tau)); q.onem_mtau = 1.0 - q.mtau;
        std::vector<double> pw(2048);               // mtau^(k + 1): the carried dc's weight at sample k of a tile (fm_audio_at)
        for (int k = 0; k < 2048; k++) pw[(size_t)k] = std::pow(q.mtau, (double)(k + 1));
        if (int rc = alloc(fm_pw, 2048)) return rc;
        QH_HIP(hipMemcpyAsync(fm_pw, pw.data(), 2048 * sizeof(double), hipMemcpyHostToDevice, stream));
        QH_HIP(hipStreamSynchronize(stream));
    }
    demod_alloc = true;
    lists_dirty = true;
    for (ChanCfg &c : cfg) c.demod_dirty = true;
    return QH_OK;
}

// Every channel list from the channels' settings (host side: h[id]), with their counts
void Engine::build_lists(std::vector<int> (&h)[L_COUNT])
{
    std::vector<int> stale_cur, stale_other;
    int sam0 = 0;
    ssql_h[0].clear(); ssql_h[1].clear();
    for (int ch = 0; ch < nch; ch++) {
        const ChanCfg &c = cfg[(size_t)ch];
        if (c.amsq_run) h[L_AMSQ].push_back(ch);
        if (c.snba_run) h[L_SNBA].push_back(ch);
        if (c.snb_pos() >= 0) h[L_SNB + c.snb_pos()].push_back(ch);
        const int at_agc = (c.bp1_run && !c.bp1_pos) ? 1 : 0;       // the buffer the channel is in when xwcpagc runs
        if (c.emnr_run) h[L_EMNR + (c.emnr_pos ? 1 + at_agc : 0)].push_back(ch);
        for (int f = 0; f < 2; f++) if (c.lms[f].run) h[L_LMS + 3 * f + (c.lms[f].position ? 1 + at_agc : 0)].push_back(ch);
        if (c.bp1_run) h[L_BP1P + (c.bp1_pos ? 1 : 0)].push_back(ch);
        if (c.fix_before()) h[L_FIX + at_agc].push_back(ch);
        if (c.ap_on()) h[L_AP + (c.bp1_run ? 1 : 0)].push_back(ch);        // where the channel is behind bp1 at either position
        if (c.ssql_on()) ssql_h[c.bp1_run ? 1 : 0].push_back(ch);
        if (c.fmd_run && c.lim_run) h[L_LIM].push_back(ch);
        if (c.amd_run && c.amd_mode == 0) h[L_AM].push_back(ch);
        // SAM channels with sbmode 0 (no all-pass chains) first
        if (c.amd_run && c.amd_mode == 1) { if (c.sbmode == 0) h[L_SAM].insert(h[L_SAM].begin() + sam0++, ch); else h[L_SAM].push_back(ch); }
        if (c.fmd_run) h[L_FM].push_back(ch); else { h[L_REST].push_back(ch); h[c.bp1_run ? L_RB : L_USB].push_back(ch); }
        h[c.bp1_run ? L_BP1 : L_PLAIN].push_back(ch);
        // xwcpagc sits between the two bp1 positions (RXA.c:581-586): a position-1 channel is still in `cur` there; channels whose
        // attack window moved in mid-stream go last
        if (c.agc_run && c.agc_mode != 0) (at_agc ? (c.agc_stale ? stale_other : h[L_AGC_OTHER]) : (c.agc_stale ? stale_cur : h[L_AGC_CUR])).push_back(ch);
    }
    n_sam0 = sam0;
    n_agc_cur_stale = (int)stale_cur.size(); n_agc_other_stale = (int)stale_other.size();
    h[L_AGC_CUR].insert(h[L_AGC_CUR].end(), stale_cur.begin(), stale_cur.end());
    h[L_AGC_OTHER].insert(h[L_AGC_OTHER].end(), stale_other.begin(), stale_other.end());
    // partners: neighbours in the list, ordered so that equal designs are neighbours; a channel left over is its own partner
    auto bp1_real = [&](int ch) { const ChanCfg &c = cfg[(size_t)ch]; return c.bp1_run && c.bp1_flow == -c.bp1_fhigh && !c.mp; };
    auto bp1_same = [&](int x, int y) {
        const ChanCfg &p = cfg[(size_t)x], &q = cfg[(size_t)y];
        return p.bp1_nc == q.bp1_nc && p.bp1_wintype == q.bp1_wintype && p.bp1_fhigh == q.bp1_fhigh && p.bp1_gain == q.bp1_gain;
    };
    auto bp1_pairs = [&](std::vector<int> v) {
        std::vector<int> pr;
        for (int ch : v) if (!bp1_real(ch)) return pr;
        std::stable_sort(v.begin(), v.end(), [&](int x, int y) {
            const ChanCfg &p = cfg[(size_t)x], &q = cfg[(size_t)y];
            if (p.bp1_fhigh != q.bp1_fhigh) return p.bp1_fhigh < q.bp1_fhigh;
            if (p.bp1_nc != q.bp1_nc) return p.bp1_nc < q.bp1_nc;
            if (p.bp1_wintype != q.bp1_wintype) return p.bp1_wintype < q.bp1_wintype;
            return p.bp1_gain < q.bp1_gain;
        });
        for (size_t i = 0; i < v.size();) {
            if (i + 1 < v.size() && bp1_same(v[i], v[i + 1])) { pr.push_back(v[i]); pr.push_back(v[i + 1]); i += 2; }
            else { pr.push_back(v[i]); pr.push_back(v[i]); i += 1; }
        }
        return pr;
    };
    const std::vector<int> &fm = h[L_FM];
    for (size_t i = 0; i < fm.size(); i += 2) { h[L_PAIRS_FM].push_back(fm[i]); h[L_PAIRS_FM].push_back(i + 1 < fm.size() ? fm[i + 1] : fm[i]); }
    h[L_PAIRS_AM] = bp1_pairs(h[L_AM]);
    h[L_PAIRS_SAM] = bp1_pairs(h[L_SAM]);
    np_fm = (int)h[L_PAIRS_FM].size() / 2; np_am = (int)h[L_PAIRS_AM].size() / 2; np_sam = (int)h[L_PAIRS_SAM].size() / 2;
    for (int i = 0; i < L_COUNT; i++) lists[i].n = (int)h[i].size();
    for (int b = 0; b < 2; b++) ssql_lists[b].n = (int)ssql_h[b].size();
}

// The stages made when a channel first runs one of them (the lists' counts say which)
int Engine::stages_alloc()
{
    const double rate = (double)dsp_rate;
    if ((lists[L_AP].n || lists[L_AP + 1].n) && !ap_prm) if (int rc = ap_alloc()) return rc;
    if (ssql_listed() && !ssql_prm) if (int rc = ssql_alloc()) return rc;
    if ((lists[L_EMNR].n || lists[L_EMNR + 1].n || lists[L_EMNR + 2].n) && !emnr_state) if (int rc = emnr_alloc()) return rc;
    if (lists[L_SNBA].n && !snba_state) if (int rc = snba_alloc()) return rc;
    if (lists[L_AMSQ].n && !amsq_prm) {
        if (int rc = alloc(amsq_prm, nch)) return rc;
        if (int rc = alloc(amsq_state, nch, true)) return rc;
        // compute_slews, amsq.c:28-46, with muted_gain 0 and 70 ms up / down (RXA.c:166-167,172): theta accumulates as there
        amsq_ntup = (int)(0.070 * rate); amsq_ntdown = (int)(0.070 * rate);
        std::vector<double> up((size_t)amsq_ntup + 1), down((size_t)amsq_ntdown + 1);
        double delta = kPiRef / (double)amsq_ntup, theta = 0.0;
        for (int i = 0; i <= amsq_ntup; i++) { up[(size_t)i] = 0.0 + (1.0 - 0.0) * 0.5 * (1.0 - std::cos(theta)); theta += delta; }
        delta = kPiRef / (double)amsq_ntdown; theta = 0.0;
        for (int i = 0; i <= amsq_ntdown; i++) { down[(size_t)i] = 0.0 + (1.0 - 0.0) * 0.5 * (1.0 + std::cos(theta)); theta += delta; }
        if (int rc = alloc(amsq_cup, (long long)up.size())) return rc;
        if (int rc = alloc(amsq_cdown, (long long)down.size())) return rc;
        QH_HIP(hipMemcpyAsync(amsq_cup, up.data(), up.size() * 8, hipMemcpyHostToDevice, stream));
        QH_HIP(hipMemcpyAsync(amsq_cdown, down.data(), down.size() * 8, hipMemcpyHostToDevice, stream));
        QH_HIP(hipStreamSynchronize(stream));
        for (ChanCfg &c : cfg) c.amsq_dirty = true;
    }
    bool any_lms = false;
    for (int k = 0; k < 6; k++) any_lms = any_lms || lists[L_LMS + k].n;
    if (any_lms && !lms_prm[0]) {
        for (int f = 0; f < 2; f++) {
            if (int rc = alloc(lms_prm[f], nch)) return rc;
            if (int rc = alloc(lms_state[f], nch)) return rc;
            // create_anf: lidx 1.0, ngamma 6.25e-12; create_anr: lidx 120.0, ngamma 0.001 (RXA.c:289-292,309-312)
            std::vector<LmsState> init((size_t)nch);
            std::memset(init.data(), 0, init.size() * sizeof(LmsState));
            for (LmsState &st : init) { st.lidx = f ? 120.0 : 1.0; st.ngamma = f ? 0.001 : 6.25e-12; }
            QH_HIP(hipMemcpyAsync(lms_state[f], init.data(), init.size() * sizeof(LmsState), hipMemcpyHostToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
        }
        for (ChanCfg &c : cfg) { c.lms[0].dirty = c.lms[1].dirty = true; c.lms[0].flush = c.lms[1].flush = false; }
    }
    if (lists[L_LIM].n && !lim_prm) {
        if (int rc = alloc(lim_prm, nch)) return rc;
        if (int rc = alloc(lim_state, nch)) return rc;
        for (ChanCfg &c : cfg) c.lim_dirty = true;
    }
    return QH_OK;
}

// A fircore keeps its delay lines while its channel is off the stage's list, and the ping-pong pair flips for the listed channels
// only: a channel that (re)joins the list finds its rows in the half that was current when it left (c.*at), and they move to the
// current one.  rows: the stage's short and long delay lines, each with the half that is current for it.
int Engine::follow_rows(std::vector<char> &listed, int ChanCfg::*at, int cur, const std::vector<int> &chans, std::initializer_list<Rows> rows)
{
    if (listed.size() != (size_t)nch) listed.assign((size_t)nch, 0);
    for (int ch = 0; ch < nch; ch++) if (listed[(size_t)ch]) cfg[(size_t)ch].*at = cur;
    std::fill(listed.begin(), listed.end(), 0);
    for (int ch : chans) {
        int &a = cfg[(size_t)ch].*at;
        if (a != cur)
            for (const Rows &r : rows)
                if (r.h[0] && r.h[1])
                    QH_HIP(hipMemcpyAsync(r.h[r.cur] + (size_t)ch * r.len, r.h[a] + (size_t)ch * r.len, (size_t)r.len * sizeof(double2),
                                          hipMemcpyDeviceToDevice, stream));
        a = cur;
        listed[(size_t)ch] = 1;
    }
    return QH_OK;
}

// setNc_fircore's flush (wdsp/firmin.c:454-466): zero n channels' delay lines from channel ch on, short and long, in both halves
int Engine::zero_rows(double2 *const h[2], double2 *const lh[2], int ch, int n)
{
    for (int i = 0; i < 2; i++) {
        QH_HIP(hipMemsetAsync(h[i] + (size_t)ch * kHistBand, 0, (size_t)n * kHistBand * sizeof(double2), stream));
        if (lh[i]) QH_HIP(hipMemsetAsync(lh[i] + (size_t)ch * kLongHist, 0, (size_t)n * kLongHist * sizeof(double2), stream));
    }
    return QH_OK;
}

// Lists, stages and delay-line rows after a setter moved a channel between lists
int Engine::refresh_lists()
{
    std::vector<int> h[L_COUNT];
    build_lists(h);
    if (int rc = stages_alloc()) return rc;
    if (snba_state) {       // bpsnba's fircore (the partitioned form's 16383-sample delay line goes along: nc > 4096)
        std::vector<int> snb(h[L_SNB]);
        snb.insert(snb.end(), h[L_SNB + 1].begin(), h[L_SNB + 1].end());
        if (int rc = follow_rows(snb_listed, &ChanCfg::snb_hist_at, cur_snb, snb, { { hist_snb, cur_snb, kHistBand }, { lhist[4], cur_snb, kLongHist } }))
            return rc;
    }
    // bp1's: SetRXABandpassRun (bandpass.c:385-390) switches it on without RXAbp1Set's flush (RXA.c:825)
    if (int rc = follow_rows(bp1_listed, &ChanCfg::bp1_hist_at, cur_bp1, h[L_BP1], { { hist_bp1, cur_bp1, kHistBand }, { lhist[1], cur_bp1, kLongHist } }))
        return rc;
    // the FM de-emphasis / audio fircores' while the channel is in another mode (SetRXAMode only clears fmd's run flag, RXA.c:758-776);
    // fm_hist_at follows the de-emphasis filter's half
    if (int rc = follow_rows(fm_listed, &ChanCfg::fm_hist_at, cur_de, h[L_FM], { { hist_de, cur_de, kHistBand }, { hist_aud, cur_aud, kHistBand },
                                                                                { lhist[2], cur_de, kLongHist }, { lhist[3], cur_aud, kLongHist } }))
        return rc;
    std::vector<int> all((size_t)nch * (L_COUNT + 3));
    for (int i = 0; i < L_COUNT; i++) std::copy(h[i].begin(), h[i].end(), all.begin() + (lists[i].dev - list_block));
    std::vector<double> fg((size_t)nch);
    for (int ch = 0; ch < nch; ch++) fg[(size_t)ch] = cfg[(size_t)ch].agc_fixed;
    QH_HIP(hipMemcpyAsync(list_block, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(fix_gain, fg.data(), fg.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    std::vector<int> ss;
    if (ssql_list_block) {
        ss.assign((size_t)nch * 2, 0);
        for (int b = 0; b < 2; b++) std::copy(ssql_h[b].begin(), ssql_h[b].end(), ss.begin() + (size_t)nch * b);
        QH_HIP(hipMemcpyAsync(ssql_list_block, ss.data(), ss.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    }
    QH_HIP(hipStreamSynchronize(stream));
    lists_dirty = false;
    return QH_OK;
}

// loadWcpAGC, wdsp/wcpAGC.c:115-146, in its order of expressions; the arguments in create_wcpagc's
static AgcParam load_wcpagc(double rate, double tau_attack, double tau_decay, double n_tau, double max_gain, double var_gain, double max_input,
                            double out_targ, double tau_fast_back, double tau_fast_decay, double pop_ratio, int hang_enable, double tau_hang_backmult,
                            double hangtime, double hang_thresh, double tau_hang_decay)
{
    AgcParam q{};
    q.attack_buffsize = (int)std::ceil(rate * n_tau * tau_attack);
    q.attack_mult = 1.0 - std::exp(-1.0 / (rate * tau_attack));
    q.decay_mult = 1.0 - std::exp(-1.0 / (rate * tau_decay));
    q.fast_decay_mult = 1.0 - std::exp(-1.0 / (rate * tau_fast_decay));
    q.fast_backmult = 1.0 - std::exp(-1.0 / (rate * tau_fast_back));
    q.onemfast_backmult = 1.0 - q.fast_backmult;
    q.out_target = out_targ * (1.0 - std::exp(-n_tau)) * 0.9999;
    q.min_volts = q.out_target / (var_gain * max_gain);
    q.inv_out_target = 1.0 / q.out_target;
    double tmp = std::log10(q.out_target / (max_input * var_gain * max_gain));
    if (tmp == 0.0) tmp = 1e-16;
    q.slope_constant = (q.out_target * (1.0 - 1.0 / var_gain)) / tmp;
    q.inv_max_input = 1.0 / max_input;
    tmp = std::pow(10.0, (hang_thresh - 1.0) / 0.125);
    q.hang_level = (max_input * tmp + (q.out_target / (var_gain * max_gain)) * (1.0 - tmp)) * 0.637;
    q.hang_backmult = 1.0 - std::exp(-1.0 / (rate * tau_hang_backmult));
    q.onemhang_backmult = 1.0 - q.hang_backmult;
    q.hang_decay_mult = 1.0 - std::exp(-1.0 / (rate * tau_hang_decay));
    q.pop_ratio = pop_ratio;
    q.hang_count_init = (int)(hangtime * rate);
    q.hang_enable = hang_enable;
    q.pmode = 1;
    return q;
}

// ---- per-channel parameters of the demodulator stages (refresh_demod: each only when its setter has run)
int Engine::prm_agc(ChanCfg &c, int ch)
{
    if (!c.agc_dirty) return QH_OK;
    // create_rxa's constants (RXA.c:335-358)
    const AgcParam q = load_wcpagc((double)dsp_rate, c.agc_tau_attack, c.agc_tau_decay, 4.0, c.agc_max_gain, c.agc_var_gain, 1.0, 1.0, 0.250, 0.005,
                                   5.0, 1, 0.500, c.agc_hangtime, c.agc_hang_thresh, 0.100);
    if (q.attack_buffsize + 2 > kAgcRing)
        return set_error(QH_ERR_UNSUPPORTED, "AGC attack of %g s needs a look-ahead of %d samples (limit %d)", c.agc_tau_attack,
                         q.attack_buffsize, kAgcRing - 2);
    c.agc_abuf = q.attack_buffsize;
    if (int rc = put_row(agc_prm, ch, q)) return rc;
    c.agc_dirty = false;
    return QH_OK;
}

int Engine::prm_emnr(ChanCfg &c, int ch)
{
    if (emnr_chan && c.emnr_dirty) {
        if (c.emnr_run && (c.emnr_npe < 0 || c.emnr_npe > 2 || c.emnr_gain_method < 0 || c.emnr_gain_method > 3))
            return set_error(QH_ERR_UNSUPPORTED, "EMNR: gain methods 0..3 and noise estimators 0..2");
        const EmnrChan ec{ c.emnr_gain_method, c.emnr_npe, c.emnr_ae, 0, c.emnr_ae_zeta, c.emnr_ae_psi, c.emnr_train_zeta, c.emnr_train_t2 };
        if (int rc = put_row(emnr_chan, ch, ec)) return rc;
        c.emnr_dirty = false;
    }
    if (emnr_state && c.emnr_flush) {           // flush_emnr, emnr.c:583-596: the accumulators and their indices, not the estimators
        EmnrScalars sc;
        QH_HIP(hipMemcpyAsync(&sc, emnr_scal + ch, sizeof(sc), hipMemcpyDeviceToHost, stream));
        QH_HIP(hipStreamSynchronize(stream));
        sc.iainidx = sc.iaoutidx = sc.oaoutidx = sc.nsamps = sc.saveidx = 0; sc.oainidx = emnr_prm.init_oainidx;
        if (int rc = put_row(emnr_scal, ch, sc, false)) return rc;
        QH_HIP(hipMemsetAsync(emnr_state + (size_t)ch * kEmnrStateDoubles, 0, (size_t)EO_PREVG * sizeof(double), stream));
        QH_HIP(hipStreamSynchronize(stream));
        c.emnr_flush = false;
    }
    return QH_OK;
}

int Engine::prm_snba(ChanCfg &c, int ch)
{
    const SnbaParam &q = snba_prm;
    if (snba_state && c.snba_taps_dirty) {
        // calc_resample for outresamp (12 kHz -> dsp_rate, gain 2, resample.c:35-79) with the channel's output bandwidth
        if (q.ratio > 1) {
            const int L = q.ratio, ncoef = q.cpp_out * L;
            const double full = (double)(12000 * L), fc = c.snba_f_high == 0.0 ? 0.45 * 12000.0 : c.snba_f_high;
            const double lo = c.snba_f_low < 0.0 ? -fc / full : c.snba_f_low / full;
            const std::vector<cd> imp = fir_bandpass(ncoef, lo, fc / full, 1.0, 1, 0, 2.0 * (double)L);
            std::vector<double> hp((size_t)ncoef);
            size_t i = 0;
            for (int j = 0; j < L; j++) for (int k = 0; k < ncoef; k += L) hp[i++] = imp[(size_t)(j + k)].real();
            QH_HIP(hipMemcpyAsync(snba_hout + (size_t)ch * ncoef, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
        }
        c.snba_taps_dirty = false;
    }
    if (snba_state && (c.snba_flush || c.snba_rout_flush)) {
        double *st = snba_state + (size_t)ch * q.state_doubles;
        if (q.cpp_out > 1) QH_HIP(hipMemsetAsync(st + q.off_rout, 0, (size_t)(q.cpp_out - 1) * sizeof(double), stream));
        if (c.snba_flush) {         // flush_snba, snb.c:161-185: the frame half of xbase, the accumulators, both resamplers
            QH_HIP(hipMemsetAsync(st + kSnbX, 0, (size_t)kSnbX * sizeof(double), stream));
            QH_HIP(hipMemsetAsync(st + q.off_inacc, 0, (size_t)(q.state_doubles - q.off_inacc) * sizeof(double), stream));
            if (int rc = put_row(snba_idx, ch, SnbaIdx{ 0, 0, 0, 0, q.init_oaoutidx, { 0, 0, 0 } })) return rc;
        }
    }
    c.snba_flush = c.snba_rout_flush = false;
    return QH_OK;
}

int Engine::prm_amsq(ChanCfg &c, int ch)
{
    if (!amsq_prm || !c.amsq_dirty) return QH_OK;
    // calc_amsq, amsq.c:48-64: 10 ms average (RXA.c:165)
    const double rate = (double)dsp_rate;
    AmsqParam q{};
    q.avm = std::exp(-1.0 / (rate * 0.010)); q.onem_avm = 1.0 - q.avm;
    q.tail_thresh = c.amsq_tail_thresh; q.unmute_thresh = c.amsq_unmute_thresh; q.min_tail = 0.0; q.max_tail = c.amsq_max_tail;
    q.muted_gain = 0.0; q.rate = rate; q.ntup = amsq_ntup; q.ntdown = amsq_ntdown;
    if (int rc = put_row(amsq_prm, ch, q)) return rc;
    c.amsq_dirty = false;
    return QH_OK;
}

int Engine::prm_lms(ChanCfg &c, int ch)
{
    for (int f = 0; f < 2 && lms_prm[0]; f++) {
        ChanCfg::Lms &m = c.lms[f];
        if (m.dirty) {
            if (m.run && (m.taps < 1 || m.taps > 64 || m.delay < 1 || m.delay > 64))
                return set_error(QH_ERR_UNSUPPORTED, "%s: taps %d / delay %d (1..64 each: one tap per lane)", f ? "ANR" : "ANF", m.taps, m.delay);
            // lidx_min, lidx_max, den_mult, lincr, ldecr of create_rxa (RXA.c:290-295,310-315)
            if (int rc = put_row(lms_prm[f], ch, LmsParam{ m.taps, m.delay, f, 0, m.two_mu, m.gamma, f ? 120.0 : 0.0, 200.0, 6.25e-10, 1.0, 3.0 }))
                return rc;
            m.dirty = false;
        }
        if (m.flush) {          // flush_anf (anf.c:135-140): delay line and weights; lidx / ngamma carry on
            QH_HIP(hipMemsetAsync(lms_state[f] + ch, 0, offsetof(LmsState, lidx), stream));
            m.flush = false;
        }
    }
    return QH_OK;
}

int Engine::prm_lim(ChanCfg &c, int ch)
{
    if (!c.lim_dirty || !lim_prm) return QH_OK;
    // calc_fmd's create_wcpagc(1, 5, 1, ..., 0.001, 0.008, 4, lim_gain, 1.0, 1.0, 1.0, 0.9, 0.250, 0.004, 4.0, 0,
    // 0.500, 0.500, 2.000, 0.100) (fmd.c:48-72) through loadWcpAGC; a new limiter starts cleared
    const AgcParam q = load_wcpagc((double)dsp_rate, 0.001, 0.008, 4.0, c.lim_gain, 1.0, 1.0, 0.9, 0.250, 0.004, 4.0, 0, 0.500, 0.500, 2.000, 0.100);
    if (int rc = put_row(lim_prm, ch, q, false)) return rc;
    QH_HIP(hipMemsetAsync(lim_state + ch, 0, sizeof(AgcState), stream));
    if (int rc = put_row(&lim_state[ch].out_index, 0, kAgcRing - 1)) return rc;        // out_index = -1 (calc_wcpagc, wcpAGC.c:34)
    c.lim_dirty = false;
    return QH_OK;
}

// the detectors' own parameters: AM's fade leveller, SAM's sideband mode, FM's gain and its CTCSS notch
int Engine::prm_detect(ChanCfg &c, int ch)
{
    if (!c.demod_dirty) return QH_OK;
    const int lf = c.levelfade;
    const double again = (double)dsp_rate / (c.fm_dev * kTwoPiRef);     // wdsp/fmd.c:44
    const SamChanParam sp{ c.sbmode, c.levelfade };
    SnotchParam sn{};
    {   // calc_snotch, wdsp/iir.c:35-49 (bw 0.0002, fmd.c:47)
        const double fn = c.ctcss_freq / (double)dsp_rate, csn = std::cos(kTwoPiRef * fn), qr = 1.0 - 3.0 * 0.0002;
        const double qk = (1.0 - 2.0 * qr * csn + qr * qr) / (2.0 * (1.0 - csn));
        sn.a0 = qk; sn.a1 = -2.0 * qk * csn; sn.a2 = qk; sn.b1 = 2.0 * qr * csn; sn.b2 = -qr * qr; sn.run = c.ctcss_run;
    }
    if (int rc = put_row(levelfade, ch, lf, false)) return rc;
    if (int rc = put_row(fm_again, ch, again, false)) return rc;
    if (int rc = put_row(sam_prm, ch, sp, false)) return rc;
    if (int rc = put_row(sn_prm, ch, sn, false)) return rc;
    if (c.ctcss_flush) {                    // calc_snotch ends with flush_snotch, wdsp/iir.c:48
        QH_HIP(hipMemsetAsync(sn_state + ch, 0, sizeof(SnotchState), stream));
        c.ctcss_flush = false;
    }
    QH_HIP(hipStreamSynchronize(stream));
    c.demod_dirty = false;
    return QH_OK;
}

// create_fmd, wdsp/fmd.c:108-116: the de-emphasis and audio filters the FM channels share, rebuilt when their nc, RXASetMP or the band
// tile moved
int Engine::fm_filters(int want_nc)
{
    if (!want_nc || (want_nc == fm_nc_built && fm_mp == fm_mp_built && fm_nfft_built == 2 * bnfft + (band2g ? 1 : 0))) return QH_OK;
    // de-emphasis by frequency sampling, audio band-pass 0.8*f_low .. 1.1*f_high
    const double rate = (double)dsp_rate, f_low = 300.0, f_high = 3000.0, afgain = 0.5;
    std::vector<cd> de = fc_impulse(want_nc, f_low, f_high, +20.0 * std::log10(f_high / f_low), 0.0, 1, rate, 1.0 / (2.0 * dsp_size), 0, 0);
    std::vector<cd> au = fir_bandpass(want_nc, 0.8 * f_low, 1.1 * f_high, rate, 0, 1, afgain / (2.0 * dsp_size));
    if (fm_mp) { de = mp_imp(de, 16, 0); au = mp_imp(au, 16, 0); }     // SetRXAFMMPde / MPaud, wdsp/RXA.c:956-957
    fm_mp_built = fm_mp;
    for (auto &v : de) v *= (double)(2 * dsp_size);
    for (auto &v : au) v *= (double)(2 * dsp_size);
    de_real = true;
    for (const cd &v : de) de_real = de_real && v.imag() == 0.0;
    if (long_parts[2] > 1) {
        if (int rc = long_masks_upload(2, 0, de)) return rc;
        if (int rc = long_masks_upload(3, 0, au)) return rc;
        de.resize((size_t)kLongPart); au.resize((size_t)kLongPart);      // (the one-tile masks are not used then)
    }
    if (int rc = upload(mask_de, band_mask(de), stream)) return rc;
    if (int rc = upload(mask_aud, band_mask(au), stream)) return rc;
    fm_nfft_built = 2 * bnfft + (band2g ? 1 : 0);
    if (fm_nc_built && fm_nc_built != want_nc) {      // setNc_fircore zeroes the delay lines
        if (int rc = zero_rows(hist_de, lhist[2], 0, nch)) return rc;
        if (int rc = zero_rows(hist_aud, lhist[3], 0, nch)) return rc;
    }
    fm_nc_built = want_nc;
    return QH_OK;
}

// Demodulator state, channel lists and FM filters (only engines that run AM/SAM/FM channels get here).  Every step looks at flags
// first: a call with nothing dirty allocates, copies and waits for nothing.
int Engine::refresh_demod()
{
    if (!demod_alloc) if (int rc = demod_init()) return rc;
    // a channel whose attack window moves after its AGC has run keeps the reference's ring_max, which may then be a value the window
    // no longer holds (wcpAGC.c:197-210 only rescans when the sample that leaves equals it): the time tiles take the window's maximum,
    // so that channel stays on the kernel that steps the reference's bookkeeping -- it alone: the lists put such channels last
    for (ChanCfg &c : cfg) {
        if (!c.agc_dirty || !c.agc_ran) continue;
        const int abuf = (int)std::ceil((double)dsp_rate * 4.0 * c.agc_tau_attack);
        if (c.agc_abuf != abuf) { c.agc_rewindow = true; if (!c.agc_stale) { c.agc_stale = true; lists_dirty = true; } }
    }
    if (lists_dirty) if (int rc = refresh_lists()) return rc;
    int want_nc = 0, want_mp = -1;
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (c.fmd_run) {
            if (want_nc && want_nc != c.fm_nc) return set_error(QH_ERR_UNSUPPORTED, "FM channels with different nc in one engine");
            want_nc = c.fm_nc;
            // RXASetMP reaches the FM filters of ITS channel (SetRXAFMMPde / MPaud, wdsp/RXA.c:956-957): the one design the engine's FM
            // channels share follows them, not whichever channel was set last
            if (want_mp >= 0 && want_mp != c.mp) return set_error(QH_ERR_UNSUPPORTED, "FM channels with different RXASetMP in one engine");
            want_mp = c.mp;
        }
        if (int rc = prm_agc(c, ch)) return rc;
        if (int rc = prm_emnr(c, ch)) return rc;
        if (int rc = prm_snba(c, ch)) return rc;
        if (int rc = prm_amsq(c, ch)) return rc;
        if (int rc = prm_lms(c, ch)) return rc;
        if (int rc = prm_lim(c, ch)) return rc;
        if (int rc = prm_detect(c, ch)) return rc;
    }
    if (want_mp >= 0) fm_mp = want_mp;
    return fm_filters(want_nc);
}

// the frame advance and the two accumulators' sizes for an overlap (calc_snba, snb.c:45-65)
void Engine::snba_plan(int ovrlp)
{
    SnbaParam &q = snba_prm;
    q.incr = kSnbX / ovrlp;
    q.iasize = q.incr > q.isize ? q.incr : q.isize;
    q.oasize = q.iasize;
    q.init_oaoutidx = q.incr > q.isize ? q.isize : 0;
    q.off_inacc = 2 * kSnbX; q.off_outacc = q.off_inacc + q.iasize; q.off_rin = q.off_outacc + q.oasize;
    q.off_rout = q.off_rin + (q.cpp_in - 1); q.state_doubles = q.off_rout + (q.cpp_out - 1);
}

// SetRXASNBAovrlp (snb.c:595-603): decalc_snba + calc_snba with the new overlap -- the frame memory (xbase, made by create_snba) stays,
// the accumulators, their indices and both resamplers start over
int Engine::snba_set_ovrlp(int ovrlp)
{
    if (ovrlp < 1 || ovrlp > kSnbX || kSnbX / ovrlp < 1) return set_error(QH_ERR_INVALID, "SetRXASNBAovrlp: 1 .. %d", kSnbX);
    snba_ovrlp = ovrlp;
    if (!snba_state) return QH_OK;                       // nothing built yet: snba_alloc plans with it
    QH_HIP(hipSetDevice(device));
    if (int rc = quiesce()) return rc;
    const SnbaParam old = snba_prm;
    std::vector<double> frames((size_t)nch * 2 * kSnbX);
    QH_HIP(hipMemcpy2D(frames.data(), 2 * kSnbX * sizeof(double), snba_state, (size_t)old.state_doubles * sizeof(double), 2 * kSnbX * sizeof(double),
                       (size_t)nch, hipMemcpyDeviceToHost));
    snba_plan(ovrlp);
    const SnbaParam &q = snba_prm;
    if (int rc = alloc(snba_state, (long long)nch * q.state_doubles)) return rc;
    QH_HIP(qh::dev_zero(snba_state, (size_t)nch * q.state_doubles * sizeof(double)));
    QH_HIP(hipMemcpy2D(snba_state, (size_t)q.state_doubles * sizeof(double), frames.data(), 2 * kSnbX * sizeof(double), 2 * kSnbX * sizeof(double),
                       (size_t)nch, hipMemcpyHostToDevice));
    std::vector<SnbaIdx> ix((size_t)nch, SnbaIdx{ 0, 0, 0, 0, q.init_oaoutidx, { 0, 0, 0 } });
    QH_HIP(hipMemcpy(snba_idx, ix.data(), ix.size() * sizeof(SnbaIdx), hipMemcpyHostToDevice));
    return QH_OK;
}

// calc_emnr (wdsp/emnr.c:240-497) with create_rxa's arguments (RXA.c:319-332): parameters, window, start values of every array
int Engine::snba_alloc()
{
    // calc_snba, snb.c:31-66, with create_rxa's arguments (RXA.c:237-255)
    SnbaParam &q = snba_prm;
    if (dsp_rate % 12000 || (dsp_rate / 12000 != 1 && dsp_rate / 12000 != 2 && dsp_rate / 12000 != 4) || dsp_size > kSnbMaxDsp ||
        dsp_size % (dsp_rate / 12000))
        return set_error(QH_ERR_UNSUPPORTED, "SNBA: dsp_rate 12000, 24000 or 48000 and dsp_size up to %d", kSnbMaxDsp);
    q.ratio = dsp_rate / 12000;
    q.isize = dsp_size / q.ratio;
    q.cpp_in = q.ratio > 1 ? 140 * q.ratio + 1 : 1;
    q.cpp_out = q.ratio > 1 ? 141 : 1;
    q.asize = 64; q.npasses = 2; q.b = 10; q.pre = 2; q.post = 2; q.k1 = 8.0; q.k2 = 20.0; q.pmultmin = 0.5;
    snba_plan(snba_ovrlp);
    if (int rc = alloc(snba_state, (long long)nch * q.state_doubles, true)) return rc;
    if (int rc = alloc(snba_idx, nch)) return rc;
    std::vector<SnbaIdx> ix((size_t)nch, SnbaIdx{ 0, 0, 0, 0, q.init_oaoutidx, { 0, 0, 0 } });
    QH_HIP(hipMemcpyAsync(snba_idx, ix.data(), ix.size() * sizeof(SnbaIdx), hipMemcpyHostToDevice, stream));
    if (int rc = alloc(snba_scratch, (long long)nch * kSnbX * kSnbX)) return rc;
    if (int rc = alloc(snba_tune, nch)) return rc;
    snba_tune_dirty = true;
    if (int rc = alloc(snba_hin, q.cpp_in)) return rc;
    if (int rc = alloc(snba_hout, (long long)nch * q.cpp_out * q.ratio)) return rc;
    std::vector<double> hin((size_t)q.cpp_in, 1.0);
    if (q.ratio > 1) {      // inresamp: dsp_rate -> 12 kHz, 250 .. 5400 Hz, gain 2 (snb.c:43-44)
        const double full = (double)dsp_rate;
        const std::vector<cd> imp = fir_bandpass(q.cpp_in, 250.0 / full, 0.45 * 12000.0 / full, 1.0, 1, 0, 2.0);
        for (int i = 0; i < q.cpp_in; i++) hin[(size_t)i] = imp[(size_t)i].real();
    }
    QH_HIP(hipMemcpyAsync(snba_hin, hin.data(), hin.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    if (int rc = alloc(mask_snb, (long long)nch * kBandNfftMax)) return rc;
    for (double2 *&h : hist_snb) if (int rc = alloc(h, (long long)nch * kHistBand, true)) return rc;
    QH_HIP(hipStreamSynchronize(stream));
    snb_listed.assign((size_t)nch, 0);
    for (ChanCfg &c : cfg) { c.snba_taps_dirty = true; c.snb_dirty = true; c.snba_flush = c.snba_rout_flush = false; c.snb_flush = false; c.snb_hist_at = cur_snb; }
    return QH_OK;
}

int Engine::emnr_alloc()
{
    if (dsp_size > kEmnrIncr) return set_error(QH_ERR_UNSUPPORTED, "EMNR: dsp_size up to %d", kEmnrIncr);
    const double rate = (double)dsp_rate, incr = (double)kEmnrIncr;
    EmnrParam &q = emnr_prm;
    auto tc = [&](double base) { const double tau = -128.0 / 8000.0 / std::log(base); return std::exp(-incr / rate / tau); };
    q.gain = 1.0 / kEmnrF / 4.0;
    q.gf1p5 = std::sqrt(kPiRef) / 2.0;
    q.alpha = tc(0.985);
    q.eps_floor = 1.0e-300; q.gamma_max = 40.0; q.xi_min = std::pow(10.0, -40.0 / 10.0); q.q = 0.2; q.gmax = 10000.0;
    q.dim_zeta = 60;
    q.z_gamma_min = h_zrange[0]; q.z_gamma_max = h_zrange[1]; q.z_xihat_min = h_zrange[2]; q.z_xihat_max = h_zrange[3];
    q.alphaCsmooth = tc(0.7); q.alphaMax = tc(0.96); q.alphaCmin = tc(0.7); q.alphaMin_max_value = tc(0.3);
    q.snrq = -incr / (0.064 * rate);
    q.betamax = tc(0.8);
    q.invQeqMax = 0.5; q.av = 2.12;
    const double Dtime = 8.0 * 12.0 * 128.0 / 8000.0;
    q.U = 8;
    q.V = (int)(0.5 + (Dtime * rate / (q.U * incr)));
    if (q.V < 4) q.V = 4;
    if ((q.U = (int)(0.5 + (Dtime * rate / (q.V * incr)))) < 1) q.U = 1;
    if (q.U > kEmnrU) return set_error(QH_ERR_UNSUPPORTED, "EMNR: %d minimum sub-windows at this rate (up to %d)", q.U, kEmnrU);
    q.D = q.U * q.V;
    {
        static const double Dvals[18] = { 1.0, 2.0, 5.0, 8.0, 10.0, 15.0, 20.0, 30.0, 40.0, 60.0, 80.0, 120.0, 140.0, 160.0, 180.0, 220.0, 260.0, 300.0 };
        static const double Mvals[18] = { 0.000, 0.260, 0.480, 0.580, 0.610, 0.668, 0.705, 0.762, 0.800, 0.841, 0.865, 0.890, 0.900, 0.910,
                                          0.920, 0.930, 0.935, 0.940 };
        auto interpM = [&](double x) {              // emnr.c:185-202
            if (x <= Dvals[0]) return Mvals[0];
            if (x >= Dvals[17]) return Mvals[17];
            int idx = 0;
            while (x >= Dvals[idx]) idx++;
            const double xllow = std::log10(Dvals[idx - 1]), xlhigh = std::log10(Dvals[idx]);
            const double frac = (std::log10(x) - xllow) / (xlhigh - xllow);
            return Mvals[idx - 1] + frac * (Mvals[idx] - Mvals[idx - 1]);
        };
        q.MofD = interpM((double)q.D); q.MofV = interpM((double)q.V);
    }
    q.invQbar_points[0] = 0.03; q.invQbar_points[1] = 0.05; q.invQbar_points[2] = 0.06; q.invQbar_points[3] = 1.0e300;
    {
        const double f[4] = { 8.0, 4.0, 2.0, 1.2 };
        for (int i = 0; i < 4; i++) {
            const double db = 10.0 * std::log10(f[i]) / (12.0 * 128 / 8000);
            q.nsmax[i] = std::pow(10.0, db / 10.0 * q.V * incr / rate);
        }
    }
    q.alpha_pow = tc(0.8); q.alpha_Pbar = tc(0.9);
    q.epsH1 = std::pow(10.0, 15.0 / 10.0); q.epsH1r = q.epsH1 / (1.0 + q.epsH1);
    {   // npl, emnr.c:458-489
        auto tl = [&](double base) { const double tau = -256.0 / (20100.0 * std::log(base)); return std::exp(-incr / (rate * tau)); };
        q.l_eta = tl(0.7); q.l_gamma = tl(0.998); q.l_beta = tl(0.8); q.l_alpha_d = tl(0.85); q.l_alpha_p = tl(0.2);
        q.delta_LF = 1000.0 / (rate / 2) * kEmnrM; q.delta_MF = 3000.0 / (rate / 2) * kEmnrM;
    }
    q.bsize = dsp_size;
    q.oasize = dsp_size > kEmnrIncr ? dsp_size : kEmnrIncr;
    q.init_oainidx = (kEmnrF - dsp_size - kEmnrIncr) % q.oasize;
    // window (calc_window, wintype 0, emnr.c:160-183)
    std::vector<double> win(kEmnrF);
    {
        const double arg = 2.0 * kPiRef / (double)kEmnrF;
        double sum = 0.0;
        for (int i = 0; i < kEmnrF; i++) { win[(size_t)i] = std::sqrt(0.54 - 0.46 * std::cos((double)i * arg)); sum += win[(size_t)i]; }
        const double inv_coherent_gain = (double)kEmnrF / sum;
        for (double &w : win) w *= inv_coherent_gain;
    }
    // start values (emnr.c:309-313,409-426,452-456)
    std::vector<double> st((size_t)kEmnrStateDoubles, 0.0);
    for (int k = 0; k < kEmnrM; k++) {
        st[(size_t)(EO_PREVG + k)] = 1.0; st[(size_t)(EO_PREVM + k)] = 1.0;
        st[(size_t)(EO_P + k)] = 0.5; st[(size_t)(EO_SIG + k)] = 0.5; st[(size_t)(EO_PBAR + k)] = 0.5; st[(size_t)(EO_PMINU + k)] = 0.5;
        st[(size_t)(EO_P2BAR + k)] = 0.25;
        st[(size_t)(EO_ACTMIN + k)] = 1.0e300; st[(size_t)(EO_ACTSUB + k)] = 1.0e300;
        for (int ku = 0; ku < kEmnrU; ku++) st[(size_t)(EO_AMB + ku * kEmnrPad + k)] = 1.0e300;
        st[(size_t)(EO_SSIG + k)] = 0.5; st[(size_t)(EO_SPBAR + k)] = 0.5;
    }
    if (int rc = alloc(emnr_state, (long long)nch * kEmnrStateDoubles)) return rc;
    if (int rc = alloc(emnr_scal, nch)) return rc;
    if (int rc = alloc(emnr_chan, nch)) return rc;
    if (int rc = alloc(emnr_window, kEmnrF)) return rc;
    if (int rc = alloc(emnr_GG, 241 * 241)) return rc;
    if (int rc = alloc(emnr_GGS, 241 * 241)) return rc;
    if (int rc = alloc(emnr_zeta, 3600)) return rc;
    if (int rc = alloc(emnr_zeta_true, 3600)) return rc;
    const EmnrScalars sc0{ 0, 0, q.init_oainidx, 0, 0, 0, q.V, 0, 1.0 };
    for (int ch = 0; ch < nch; ch++) {
        QH_HIP(hipMemcpyAsync(emnr_state + (size_t)ch * kEmnrStateDoubles, st.data(), st.size() * 8, hipMemcpyHostToDevice, stream));
        QH_HIP(hipMemcpyAsync(emnr_scal + ch, &sc0, sizeof(sc0), hipMemcpyHostToDevice, stream));
    }
    QH_HIP(hipMemcpyAsync(emnr_window, win.data(), win.size() * 8, hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(emnr_GG, h_GG.data(), h_GG.size() * 8, hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(emnr_GGS, h_GGS.data(), h_GGS.size() * 8, hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(emnr_zeta, h_zeta.data(), h_zeta.size() * 8, hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(emnr_zeta_true, h_zeta_true.data(), h_zeta_true.size() * 4, hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));
    QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&emnr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, emnr_lds_bytes()));
    for (ChanCfg &c : cfg) { c.emnr_dirty = true; c.emnr_flush = false; }
    return QH_OK;
}

int Engine::ensure_buffers(long long n_mid)
{
    if (n_mid <= buf_cap) return QH_OK;
    if (int rc = quiesce()) return rc;
    for (double2 *&b : buf)
        if (int rc = alloc(b, n_mid * nch)) return rc;
    buf_cap = n_mid;
    return QH_OK;
}

// chunk partials of the fused meters: whole tiles per channel (a tile's store is not bounds-checked)
// the mask of a fircore stage for the tile in use; the two-group tile reads even bins in group A, odd bins in group B
std::vector<cd> Engine::band_mask(const std::vector<cd> &h) const
{
    std::vector<cd> m = make_mask(h, bnfft);
    if (!band2g) return m;
    std::vector<cd> p(m.size());
    const size_t half = m.size() / 2;
    for (size_t k = 0; k < half; k++) { p[k] = m[2 * k]; p[half + k] = m[2 * k + 1]; }
    return p;
}

int Engine::ensure_meter_partials(long long n_mid, int lout)
{
    const long long need = ((n_mid + lout - 1) / lout) * (lout / 64);
    if (need <= m_part_cap) return QH_OK;
    if (int rc = quiesce()) return rc;
    for (double2 *&m : m_part)
        if (int rc = alloc(m, need * nch)) return rc;
    m_part_cap = need;
    return QH_OK;
}

int Engine::ensure_abuf(long long n)
{
    return grow(abuf, abuf_cap, n, nch);
}

void Engine::pack_audio(const double2 *src, long long src_stride, long long n)
{
    const long long per = (n + 255) / 256;
    hipLaunchKernelGGL(egress_pack_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)nch), dim3(256), 0, stream, src, src_stride,
                       (int)n, eg);
}

void Engine::tick(int cat)
{
    if (!timing) return;
    if (ev_used >= (int)ev.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        ev.push_back(e);
        ev_cat.push_back(0);
    }
    ev_cat[(size_t)ev_used] = cat;
    (void)hipEventRecord(ev[(size_t)ev_used], stream);
    ev_used++;
}

template <int D, bool MIX, bool PACKED = false, bool METER = false, bool OUTMIX = false, bool EGRESS = false, int NFFT = kNfft, bool POLY = false,
          int DET = 0, bool PAIR = false>
static void launch_osfir(OsfirArgs<double> a, int ntiles, int nch, hipStream_t s)
{
    a.ntiles = ntiles;
    dim3 grid((unsigned)ntiles * (unsigned)nch), block(NT);      // 1-D: the kernel maps ids to (channel, tile), qh_osfir.hpp
    constexpr int lds = osfir_lds_bytes<double, NFFT, D, METER>();
    hipLaunchKernelGGL((osfir_kernel<double, NFFT, D, MIX, PACKED, METER, OUTMIX, EGRESS, POLY, DET, PAIR>), grid, block, lds, s, a);
}
template <int NFFT>
static void launch_band(OsfirArgs<double> a, int ntiles, int nch, hipStream_t s, bool meter, bool egress)
{
    if (meter && egress) launch_osfir<1, false, false, true, false, true, NFFT>(a, ntiles, nch, s);
    else if (meter) launch_osfir<1, false, false, true, false, false, NFFT>(a, ntiles, nch, s);
    else if (egress) launch_osfir<1, false, false, false, false, true, NFFT>(a, ntiles, nch, s);
    else launch_osfir<1, false, false, false, false, false, NFFT>(a, ntiles, nch, s);
}

static void launch_band6k(OsfirArgs<double> a, int ntiles, int nch, hipStream_t s, bool meter, bool egress)
{
    a.ntiles = ntiles;
    dim3 grid((unsigned)ntiles * (unsigned)nch), block(kOsfir6kThreads);
    constexpr int lds = osfir6k_lds_bytes();
    if (meter && egress) hipLaunchKernelGGL((osfir6k_kernel<true, true>), grid, block, lds, s, a);
    else if (meter) hipLaunchKernelGGL((osfir6k_kernel<true, false>), grid, block, lds, s, a);
    else if (egress) hipLaunchKernelGGL((osfir6k_kernel<false, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((osfir6k_kernel<false, false>), grid, block, lds, s, a);
}

static void launch_band2g(OsfirArgs<double> a, int ntiles, int nch, hipStream_t s, bool meter, bool egress)
{
    a.ntiles = ntiles;
    dim3 grid((unsigned)ntiles * (unsigned)nch), block(kOsfir8kThreads);
    constexpr int lds = osfir8k_lds_bytes();
    if (meter && egress) hipLaunchKernelGGL((osfir8k_kernel<true, true>), grid, block, lds, s, a);
    else if (meter) hipLaunchKernelGGL((osfir8k_kernel<true, false>), grid, block, lds, s, a);
    else if (egress) hipLaunchKernelGGL((osfir8k_kernel<false, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((osfir8k_kernel<false, false>), grid, block, lds, s, a);
}

// ---- stage helpers ---------------------------------------------------------------------------
// front: xshift + xresample(in) over all channels
// part 0: the whole stage.  The mixed-mode path runs the FM channels and the others on two streams: part 1 = the oscillator's tile
// table for every channel, part 2 = the tile kernel for the listed channels (on whatever `stream` is at the moment), part 3 = the
// history rows and the oscillator phases of every channel.  Parts 1 - 3 exist for the overlap-save form (D > 1) only.
int Engine::run_front(const double2 *src, long long src_stride, double2 *dst, long long dst_stride, const EpiParam *ep,
                      long long n_in, long long n_mid, const int *list, int nlist, int part)
{
    if (part == 0) tick(0);
    if (D > 1) {
        OsfirArgs<double> a{};
        a.in = src; a.in_stride = src_stride;
        a.hist = hist_front[cur_front]; a.hist_stride = kHistFront; a.hist_len = kHistFront;
        a.out = dst; a.out_stride = dst_stride; a.out_offset = 0;
        a.mask = mask_front; a.mask_stride = kNfft;
        a.tw_fwd = tw4096; a.tw_inv = tw_inv_front;
        a.nco_step = nco_step; a.lane_rot = lane_rot;
        a.epi = ep;
        a.n_in = (int)n_in; a.n_out = (int)n_mid; a.off = 0; a.P = front_P; a.Lout = front_L; a.pick = front_pick;
        const int per_tile = front_L / front_pick;
        const int ntiles = (int)((n_mid + per_tile - 1) / per_tile);
        a.chan_list = list;
        const int nl = list ? nlist : nch;
        if (part <= 1) if (int rc = grow(tile_rot, tile_rot_cap, ntiles, nch)) return rc;
        // oscillator phasor at the first input index of every tile: g0 = off - P + tile * fold * Lout (qh_osfir.hpp)
        if (part <= 1) hipLaunchKernelGGL(nco_tile_kernel, dim3((unsigned)((ntiles + 255) / 256), (unsigned)nch), dim3(256), 0, stream,
                           (const unsigned long long *)nco_phase, (const unsigned long long *)nco_dphase, tile_rot, ntiles,
                           (long long)(a.off - a.P), (long long)front_fold * front_L);
        a.tile_rot = tile_rot;
        a.pk_src = pk_src; a.pk = pk;
        // a call at least one delay line long: the tiles that hold its tail leave the next call's line (OsfirArgs::hist_next), every channel
        // in the pass of its own list
        const bool hist_in_kernel = !pk_src && n_in >= kHistFront && n_mid > 0;
        if (hist_in_kernel) a.hist_next = hist_front[cur_front ^ 1];
        if (part == 1 || part == 3) { }
        else if (pk_src) {
            switch (front_fold) {
            case 2: launch_osfir<2, false, true, false, true, false, kNfft, true>(a, ntiles, nl, stream); break;
            case 4: launch_osfir<4, false, true, false, true, false, kNfft, true>(a, ntiles, nl, stream); break;
            case 8: launch_osfir<8, false, true, false, true, false, kNfft, true>(a, ntiles, nl, stream); break;
            default: return set_error(QH_ERR_UNSUPPORTED, "decimation %d not supported", D);
            }
        } else {
            switch (front_fold) {
            case 2: launch_osfir<2, false, false, false, true, false, kNfft, true>(a, ntiles, nl, stream); break;
            case 4: launch_osfir<4, false, false, false, true, false, kNfft, true>(a, ntiles, nl, stream); break;
            case 8: launch_osfir<8, false, false, false, true, false, kNfft, true>(a, ntiles, nl, stream); break;
            default: return set_error(QH_ERR_UNSUPPORTED, "decimation %d not supported", D);
            }
        }
        if (part == 0) tick(2);
        if (part == 1 || part == 2) return QH_OK;
        dim3 g((kHistFront + NT - 1) / NT, (unsigned)nch);
        if (pk_src)
            hipLaunchKernelGGL((hist_update_kernel<double, false, true>), g, dim3(NT), 0, stream, src, src_stride, (int)n_in,
                               hist_front[cur_front], hist_front[cur_front ^ 1], kHistFront, (const unsigned long long *)nullptr,
                               (const unsigned long long *)nullptr, (const int *)nullptr, pk_src, pk);
        else if (!hist_in_kernel)
            hipLaunchKernelGGL((hist_update_kernel<double, false>), g, dim3(NT), 0, stream, src, src_stride, (int)n_in,
                               hist_front[cur_front], hist_front[cur_front ^ 1], kHistFront, (const unsigned long long *)nullptr,
                               (const unsigned long long *)nullptr, (const int *)nullptr, (const unsigned char *)nullptr, PackedFmt{});
        cur_front ^= 1;
    } else if (D == 0) {
        // any other ratio: xshift into the staging rows, then the polyphase resampler (its ring and phase live in qh_rat)
        if (pk_src) return set_error(QH_ERR_UNSUPPORTED, "packed input needs in_rate / dsp_rate in 2, 4, 8, 16");
        if (int rc = grow(fbuf, fbuf_cap, n_in, nch)) return rc;
        long long per = (n_in + NT - 1) / NT;
        dim3 g((unsigned)(per < 4096 ? per : 4096), (unsigned)nch);
        hipLaunchKernelGGL((pointwise_kernel<double, true>), g, dim3(NT), 0, stream, src, src_stride, fbuf, fbuf_cap,
                           (int)n_in, nco_phase, nco_dphase, (const EpiParam *)nullptr, (const int *)nullptr);
        int got = 0;
        if (int rc = qh_rat_process(rsmpin, fbuf, fbuf_cap, (int)n_in, dst, dst_stride, &got)) return rc;
        if (got != (int)n_mid) return set_error(QH_ERR_HIP, "input resampler produced %d samples, expected %lld", got, n_mid);
        if (ep) {       // the front stage is the chain's last: fixed AGC gain and panel, in place
            long long pm = (n_mid + NT - 1) / NT;
            hipLaunchKernelGGL((pointwise_kernel<double, false>), dim3((unsigned)(pm < 1024 ? pm : 1024), (unsigned)nch), dim3(NT), 0, stream,
                               (const double2 *)dst, dst_stride, dst, dst_stride, (int)n_mid, (const unsigned long long *)nullptr,
                               (const unsigned long long *)nullptr, ep, (const int *)nullptr);
        }
        tick(2);
    } else {
        if (pk_src) return set_error(QH_ERR_UNSUPPORTED, "packed input needs in_rate > dsp_rate (unpack with qh_unpack_iq first)");
        long long per = (n_in + NT - 1) / NT;
        dim3 g((unsigned)(per < 4096 ? per : 4096), (unsigned)nch);
        hipLaunchKernelGGL((pointwise_kernel<double, true>), g, dim3(NT), 0, stream, src, src_stride, dst, dst_stride,
                           (int)n_in, nco_phase, nco_dphase, ep, (const int *)nullptr);
        tick(2);
    }
    hipLaunchKernelGGL(nco_advance_kernel, dim3((nch + 255) / 256), dim3(256), 0, stream, nco_phase, nco_dphase, nch, n_in);
    return QH_OK;
}

// ---- impulse responses longer than 4096 taps (kLongPart) -------------------------------------------------------------------
// lcat[ch] = [the stage's last kLongHist input samples | this call's block]
// (lh = the samples of history the stage's partitions look back over, 4096 K - 1: the rows hold kLongHist, what lies further back is not moved)
static __global__ __launch_bounds__(NT) void long_gather_kernel(const double2 *hist, const double2 *src, long long src_stride, int n, double2 *cat,
                                                                long long cat_stride, const int *chan_list, int lh)
{
    const int ch = chan_list ? chan_list[blockIdx.y] : (int)blockIdx.y;
    const double2 *h = hist + (long long)ch * kLongHist, *x = src + (long long)ch * src_stride;
    double2 *c = cat + (long long)ch * cat_stride;
    const long long tot = (long long)kLongHist + n;
    for (long long i = (long long)(kLongHist - lh) + (long long)blockIdx.x * NT + threadIdx.x; i < tot; i += (long long)gridDim.x * NT) c[i] = i < kLongHist ? h[i] : x[i - kLongHist];
}
// the history the next call finds: the last kLongHist samples of lcat
static __global__ __launch_bounds__(NT) void long_hist_kernel(const double2 *cat, long long cat_stride, int n, double2 *hist, const int *chan_list, int lh)
{
    const int ch = chan_list ? chan_list[blockIdx.y] : (int)blockIdx.y;
    const double2 *c = cat + (long long)ch * cat_stride + n;
    double2 *h = hist + (long long)ch * kLongHist;
    for (int i = kLongHist - lh + blockIdx.x * NT + threadIdx.x; i < kLongHist; i += gridDim.x * NT) h[i] = c[i];
}
// partition p is added only where the channel's own impulse response reaches it (row_parts: per mask row, row_stride 0 for a shared mask)
static __global__ __launch_bounds__(NT) void long_add_kernel(double2 *dst, long long dst_stride, const double2 *add, long long add_stride, int n, const int *chan_list,
                                                             const int *row_parts, int row_stride, int p)
{
    const int ch = chan_list ? chan_list[blockIdx.y] : (int)blockIdx.y;
    if (p >= row_parts[(long long)ch * row_stride]) return;
    double2 *d = dst + (long long)ch * dst_stride;
    const double2 *a = add + (long long)ch * add_stride;
    for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) { d[i].x += a[i].x; d[i].y += a[i].y; }
}

// a stage changes between the one-tile form and the partitioned one because ONE channel's nc moved: the other channels' delay lines go
// along (the 4095 samples of the short history are the tail of the long one; the channel whose nc moved is flushed afterwards, as
// setNc_fircore does)
static __global__ __launch_bounds__(NT) void long_migrate_kernel(double2 *hist, double2 *lhist, int to_long)
{
    const int ch = blockIdx.y;
    double2 *h = hist + (long long)ch * kHistBand, *l = lhist + (long long)ch * kLongHist;
    for (int i = blockIdx.x * NT + threadIdx.x; i < kLongHist; i += gridDim.x * NT) {
        const int j = i - (kLongHist - kHistBand);
        if (to_long) l[i] = j >= 0 ? h[j] : make_double2(0.0, 0.0);
        else if (j >= 0) h[j] = l[i];
    }
}

int Engine::long_stage_alloc(int sid, bool shared_mask)
{
    if (lmask[sid]) return QH_OK;
    if (int rc = quiesce()) return rc;
    const long long rows = shared_mask ? 1 : nch;
    if (int rc = alloc(lmask[sid], rows * kLongParts * kBandNfftMax, true)) return rc;
    if (int rc = alloc(lrow_parts[sid], rows, true)) return rc;
    for (double2 *&h : lhist[sid]) if (int rc = alloc(h, (long long)nch * kLongHist, true)) return rc;
    return QH_OK;
}
int Engine::long_buffers()
{
    if (lcat && lcat_cap == buf_cap) return QH_OK;
    if (int rc = quiesce()) return rc;
    if (int rc = alloc(lcat, nch * (kLongHist + buf_cap))) return rc;
    if (int rc = alloc(ltmp, nch * buf_cap)) return rc;
    lcat_cap = buf_cap;
    return QH_OK;
}
// the kLongParts partition masks of the impulse response h (8192-point spectra of its 4096-tap slices; the slices past its end zero)
int Engine::long_masks_upload(int sid, long long row, const std::vector<cd> &h)
{
    std::vector<cd> all((size_t)kLongParts * kBandNfftMax, cd(0.0, 0.0));
    const int own = (int)std::min<size_t>((h.size() + kLongPart - 1) / kLongPart, (size_t)kLongParts);
    for (int p = 0; p < own; p++) {
        const size_t a = (size_t)p * kLongPart, b = std::min(h.size(), a + (size_t)kLongPart);
        const std::vector<cd> m = make_mask(std::vector<cd>(h.begin() + (long)a, h.begin() + (long)b), kBandNfftMax);
        std::copy(m.begin(), m.end(), all.begin() + (long)((size_t)p * kBandNfftMax));
    }
    QH_HIP(hipMemcpyAsync(lmask[sid] + (size_t)row * kLongParts * kBandNfftMax, all.data(), all.size() * sizeof(cd), hipMemcpyHostToDevice, stream));
    return put_row(lrow_parts[sid], row, own);
}

// one fircore stage (overlap-save, D = 1) over all channels (list == nullptr) or a sub-set
void Engine::run_band(const double2 *src, long long src_stride, double2 *dst, long long dst_stride, const EpiParam *ep,
                      long long n_mid, const double2 *mask, long long mask_stride, double2 **hist, int &hc, int P,
                      const int *list, int nlist, bool meter, bool egress, int det, double *det_out, long long det_stride,
                      const int *pairs, int npairs)
{
    const int sid = hist == hist_nbp ? 0 : hist == hist_bp1 ? 1 : hist == hist_de ? 2 : hist == hist_aud ? 3 : 4;
    if (long_parts[sid] > 1) {
        // nc > 4096: y = sum_p h_p * (x delayed by 4096 p).  lcat holds the stage's last 16383 samples and the block in one row per
        // channel, so partition p is the ordinary tile pass (4096 taps, 8192 points, 4097 outputs per tile) over a row that begins
        // 4096 p samples further back; the partitions' outputs are added, the epilogue follows as a pass of its own.  (The callers
        // switch every fusion off for such a call: no meters, audio frames or detector steps in this stage's stores.)
        const int K = long_parts[sid], Pk = kLongPart - 1, Lk = kBandNfftMax - Pk, nt = (int)((n_mid + Lk - 1) / Lk);
        const int nl = list ? nlist : nch;
        const long long cat_stride = kLongHist + lcat_cap;
        // what the K partitions look back over.  A channel's own nc may be shorter: the partitions past its own impulse response are not
        // added to its output (long_add_kernel), so it never depends on its row beyond its own nc -- what lies there may be an earlier,
        // longer form's samples or a non-finite burst this channel had, and a zero mask would not cancel that (NaN * 0 = NaN).
        // (The tile pass of such a partition still runs for that channel and its result is dropped: wasted work, not wrong; per-partition
        // channel lists would save it.)
        const int lh = K * kLongPart - 1;
        const long long per = (lh + n_mid + NT - 1) / NT;
        tick(1);
        hipLaunchKernelGGL(long_gather_kernel, dim3((unsigned)(per < 2048 ? per : 2048), (unsigned)nl), dim3(NT), 0, stream, (const double2 *)lhist[sid][hc], src,
                           src_stride, (int)n_mid, lcat, cat_stride, list, lh);
        for (int p = 0; p < K; p++) {
            OsfirArgs<double> a{};
            a.in = lcat + kLongHist - (long long)kLongPart * p; a.in_stride = cat_stride;
            a.hist = a.in - Pk; a.hist_stride = cat_stride; a.hist_len = Pk;
            a.out = p ? ltmp : dst; a.out_stride = p ? lcat_cap : dst_stride; a.out_offset = 0;
            a.mask = lmask[sid] + (size_t)p * kBandNfftMax; a.mask_stride = mask_stride ? (long long)kLongParts * kBandNfftMax : 0;
            a.tw_fwd = a.tw_inv = tw8192;
            a.tw_r2 = tw8192 + 32;
            a.chan_list = list;
            a.n_in = (int)n_mid; a.n_out = (int)n_mid; a.off = 0; a.P = Pk; a.Lout = Lk;
            launch_band<kBandNfftMax>(a, nt, nl, stream, false, false);
            const long long pn = (n_mid + NT - 1) / NT;
            if (p) hipLaunchKernelGGL(long_add_kernel, dim3((unsigned)(pn < 1024 ? pn : 1024), (unsigned)nl), dim3(NT), 0, stream, dst, dst_stride,
                                      (const double2 *)ltmp, lcat_cap, (int)n_mid, list, (const int *)lrow_parts[sid], mask_stride ? 1 : 0, p);
        }
        const long long pn = (n_mid + NT - 1) / NT;
        if (ep) hipLaunchKernelGGL((pointwise_kernel<double, false>), dim3((unsigned)(pn < 1024 ? pn : 1024), (unsigned)nl), dim3(NT), 0, stream,
                                   (const double2 *)dst, dst_stride, dst, dst_stride, (int)n_mid, (const unsigned long long *)nullptr,
                                   (const unsigned long long *)nullptr, ep, list);
        tick(2);
        hipLaunchKernelGGL(long_hist_kernel, dim3(64, (unsigned)nl), dim3(NT), 0, stream, (const double2 *)lcat, cat_stride, (int)n_mid, lhist[sid][hc ^ 1], list, lh);
        hc ^= 1;
        return;
    }
    const int Lout = bnfft - P;
    const int ntiles = (int)((n_mid + Lout - 1) / Lout);
    OsfirArgs<double> a{};
    a.in = src; a.in_stride = src_stride;
    a.hist = hist[hc]; a.hist_stride = kHistBand; a.hist_len = kHistBand;
    a.out = dst; a.out_stride = dst_stride; a.out_offset = 0;
    a.mask = mask; a.mask_stride = mask_stride;
    a.tw_fwd = a.tw_inv = (bnfft == kNfft || band2g) ? tw4096 : tw8192;
    a.tw_r2 = tw8192 + 32;                  // second pass table of the 8192-point plan: exp(-2 pi i k / 8192), k < 256 (qh_design.cpp)
    a.epi = ep;
    a.chan_list = list;
    a.n_in = (int)n_mid; a.n_out = (int)n_mid; a.off = 0; a.P = P; a.Lout = Lout;
    tick(1);
    if (meter) { a.meter_in = m_part[0]; a.meter_out = m_part[1]; a.meter_stride = m_part_cap; a.meter_w = m_w; }
    if (egress) a.eg = eg;
    const int nl = list ? nlist : nch;
    // the one-group tile kernel writes the next call's delay line itself when the call is at least one line long (OsfirArgs::hist_next)
    const bool hist_in_kernel = !pairs && (det || (!band6k && !band2g)) && n_mid >= kHistBand;
    if (hist_in_kernel) a.hist_next = hist[hc ^ 1];
    if (pairs) {            // the caller has checked: real taps, one mask per pair, 4096-point tiles, no meters, no egress
        a.chan_list = pairs;
        if (band_fmdc) {    // behind xfmd's loop in its local-dc form: the samples are made in the load (OsfirArgs::fmdc_*)
            a.fmdc_a = band_fmdc->a; a.fmdc_stride = band_fmdc->stride; a.fmdc_shift = band_fmdc->shift;
            a.fmdc_cin = fm_cin; a.fmdc_cstride = fm_cin_cap; a.fmdc_pw = fm_pw; a.fmdc_gain = fm_again;
        }
        if (band_amlv) {    // behind an nbp0 stage that left the envelope and the leveller's local share (DET 3)
            a.amlv_a = band_amlv->a; a.amlv_stride = band_amlv->stride; a.amlv_shift = band_amlv->shift;
            a.amlv_cin = am_cin; a.amlv_cstride = am_cin_cap; a.amlv_pw = am_pw;
        }
        launch_osfir<1, false, false, false, false, false, kNfft, false, 0, true>(a, ntiles, npairs, stream);
    } else if (det) {       // the caller has checked: 4096-point tiles, no meters, no egress
        a.det_out = det_out; a.det_stride = det_stride;
        if (det == 2 || det == 3) {
            a.det_sum = am_tsum; a.det_sum_stride = am_tsum_cap;
            a.det_m[0] = am_prm.mtauR; a.det_m[1] = am_prm.mtauI;
            a.det_m256[0] = std::pow(am_prm.mtauR, 256.0); a.det_m256[1] = std::pow(am_prm.mtauI, 256.0);
            a.det_g[0] = am_prm.onem_mtauR; a.det_g[1] = am_prm.onem_mtauI;
            a.det_lf = levelfade; a.det_last = am_last; a.det_scan = am_pw + 2 * 2048;
            for (int f = 0; f < 2; f++) {
                const double m = a.det_m[f];
                a.det_mp[f][0] = m; a.det_mp[f][1] = m * m; a.det_mp[f][2] = (m * m) * (m * m); a.det_mp[f][3] = ((m * m) * (m * m)) * ((m * m) * (m * m));
            }
            if (det == 3) launch_osfir<1, false, false, false, false, false, kNfft, false, 3>(a, ntiles, nl, stream);
            else launch_osfir<1, false, false, false, false, false, kNfft, false, 2>(a, ntiles, nl, stream);
        } else launch_osfir<1, false, false, false, false, false, kNfft, false, 1>(a, ntiles, nl, stream);
    } else if (band6k) launch_band6k(a, ntiles, nl, stream, meter, egress);
    else if (band2g) launch_band2g(a, ntiles, nl, stream, meter, egress);
    else if (bnfft == kNfft) launch_band<kNfft>(a, ntiles, nl, stream, meter, egress);
    else launch_band<kBandNfftMax>(a, ntiles, nl, stream, meter, egress);
    tick(2);
    dim3 g((kHistBand + NT - 1) / NT, (unsigned)(list ? nlist : nch));
    if (pairs && band_amlv)
        hipLaunchKernelGGL(am_audio_hist_kernel, g, dim3(256), 0, stream, band_amlv->a, band_amlv->stride, (int)n_mid, list, (const double *)am_cin, am_cin_cap,
                           (const double *)am_pw, band_amlv->shift, (const double2 *)hist[hc], hist[hc ^ 1], kHistBand);
    else if (pairs && band_fmdc)
        hipLaunchKernelGGL(fm_audio_hist_kernel, g, dim3(256), 0, stream, band_fmdc->a, band_fmdc->stride, (int)n_mid, list, (const double *)fm_cin, fm_cin_cap,
                           (const double *)fm_pw, band_fmdc->shift, (const double *)fm_again, (const double2 *)hist[hc], hist[hc ^ 1], kHistBand);
    else if (!hist_in_kernel)
        hipLaunchKernelGGL((hist_update_kernel<double, false>), g, dim3(NT), 0, stream, src, src_stride, (int)n_mid,
                           hist[hc], hist[hc ^ 1], kHistBand, (const unsigned long long *)nullptr,
                           (const unsigned long long *)nullptr, list);
    // (a listed stage reads and writes the history rows of its own channels only)
    hc ^= 1;
}

// xrxa's last step (wdsp/RXA.c:596): rsmpout runs when out_rate != dsp_rate (RXAResCheck, RXA.c:789-798)
int Engine::process(const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk)
{
    if (!rsmpout) return process_chain(d_in, in_stride, d_out, out_stride, nblk);
    if (nblk <= 0) return QH_OK;
    QH_HIP(hipSetDevice(device));
    if (eg.kind) {      // audio frames behind the output resampler: resample into the staging rows, then narrow
        const long long n_out = (long long)nblk * dsp_outsize;
        if (int rc = ensure_abuf(n_out)) return rc;
        const EgressFmt keep = eg;
        eg = EgressFmt{};
        const int rc = process(d_in, in_stride, reinterpret_cast<double *>(abuf), abuf_cap, nblk);
        eg = keep;
        if (rc) return rc;
        pack_audio(abuf, abuf_cap, n_out);
        QH_HIP(hipGetLastError());
        return QH_OK;
    }
    const long long n_mid = (long long)nblk * dsp_size;
    if (int rc = grow(obuf, obuf_cap, n_mid, nch)) return rc;
    if (int rc = process_chain(d_in, in_stride, reinterpret_cast<double *>(obuf), obuf_cap, nblk)) return rc;
    int got = 0;
    if (int rc = qh_rat_process(rsmpout, obuf, obuf_cap, (int)n_mid, d_out, out_stride, &got)) return rc;
    if (got != nblk * dsp_outsize) return set_error(QH_ERR_HIP, "output resampler produced %d samples, expected %d", got, nblk * dsp_outsize);
    return QH_OK;
}

// The chains' transition over a segment: the one-sample map of the 17 words (ds, x_j[n-1], x_j[n-2]; input 0) raised to the segment's
// length, for the two lengths a call of n samples in S segments has (q and q + 1 batches of 64), chains a / c (coefficients c0, input
// one sample late through ds) and b / d (c1).  Long double on the host; kept until the call shape changes.
int Engine::set_sb_phi(long long n, int S)
{
    const long long key = n * 1024 + S;
    if (key == sb_phi_key) return QH_OK;
    static const long double c0[7] = { -0.328201924180698L, -0.744171491539427L, -0.923022915444215L, -0.978490468768238L,
                                       -0.994128272402075L, -0.998458978159551L, -0.999790306259206L };
    static const long double c1[7] = { -0.0991227952747244L, -0.565619728761389L, -0.857467122550052L, -0.959123933111275L,
                                       -0.988739372718090L, -0.996959189310611L, -0.999282492800792L };
    constexpr int W = 17;
    typedef std::vector<long double> Mat;
    auto mul = [&](const Mat &a, const Mat &b) {
        Mat r((size_t)W * W, 0.0L);
        for (int i = 0; i < W; i++)
            for (int k = 0; k < W; k++) {
                const long double v = a[(size_t)i * W + k];
                if (v != 0.0L) for (int j = 0; j < W; j++) r[(size_t)i * W + j] += v * b[(size_t)k * W + j];
            }
        return r;
    };
    auto one_step = [&](const long double *c, bool delayed) {
        Mat m((size_t)W * W, 0.0L);
        for (int col = 0; col < W; col++) {
            long double v[W] = { 0 }, x[8];
            v[col] = 1.0L;
            x[0] = delayed ? v[0] : 0.0L;                               // the chain's input: ds (a, c) or the external input, 0 here
            for (int j = 0; j < 7; j++) x[j + 1] = c[j] * (x[j] - v[2 + 2 * (j + 1)]) + v[2 + 2 * j];       // amd.c:172-175
            long double nv[W];
            nv[0] = 0.0L;
            for (int j = 0; j < 8; j++) { nv[1 + 2 * j] = x[j]; nv[2 + 2 * j] = v[1 + 2 * j]; }
            for (int r = 0; r < W; r++) m[(size_t)r * W + col] = nv[r];
        }
        return m;
    };
    auto power = [&](Mat b, long long e) {
        Mat r((size_t)W * W, 0.0L);
        for (int i = 0; i < W; i++) r[(size_t)i * W + i] = 1.0L;
        while (e > 0) { if (e & 1) r = mul(b, r); b = mul(b, b); e >>= 1; }
        return r;
    };
    const long long q = ((n + 63) / 64) / S;
    std::vector<double> h((size_t)2 * 2 * W * W);
    for (int li = 0; li < 2; li++)
        for (int set = 0; set < 2; set++) {
            const Mat p = power(one_step(set ? c1 : c0, set == 0), 64 * (q + li));
            for (int i = 0; i < W * W; i++) h[((size_t)li * 2 + set) * W * W + i] = (double)p[(size_t)i];
        }
    if (!sb_phi) {
        if (int rc = alloc(sb_phi, (long long)h.size())) return rc;
        if (int rc = alloc(sb_sum, (long long)nch * kSegWaves * kSegMaxGroups * kSbSum)) return rc;
        if (int rc = alloc(sb_start, (long long)nch * kSegWaves * kSegMaxGroups * kSbSum)) return rc;
    }
    if (int rc = quiesce()) return rc;
    QH_HIP(hipMemcpy(sb_phi, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    sb_phi_key = key;
    return QH_OK;
}

// Whether two matrices of nch rows lie apart.  The extents are the rows' own: first sample of the first row to last sample of the last.
// (nch * stride from a pointer INTO a matrix -- a caller walking along its rows call by call -- reaches past the matrix's end by the
// offset, and whether that touches the other matrix depended on where the allocator had put the two: the same calls took one form or
// the other -- AM channels' last bits, tests/test_gpu_properties_fullsize.py -- by address.)
static bool extents_apart(const double2 *a, long long a_stride, long long a_n, const double2 *b, long long b_stride, long long b_n, int nch)
{
    const double2 *a_end = a + (size_t)(nch - 1) * (size_t)a_stride + (size_t)a_n, *b_end = b + (size_t)(nch - 1) * (size_t)b_stride + (size_t)b_n;
    return (const char *)a_end <= (const char *)b || (const char *)b_end <= (const char *)a;
}

// what the chain of every channel needs
int Engine::chain_needs(ChainCall &k)
{
    for (const ChanCfg &c : cfg) {
        if (c.agc_run && c.agc_mode > 4)
            return set_error(QH_ERR_UNSUPPORTED, "AGC mode %d is not provided (0 fixed, 1-4 long/slow/med/fast)", c.agc_mode);
        // (SetRXAAMDRun can switch the AM detector on beside the FM one, RXA.c:594-595 then runs both in a row: not provided, and said so)
        if (c.amd_run && c.fmd_run) return set_error(QH_ERR_UNSUPPORTED, "channel %d: the AM and the FM detector both switched on", (int)(&c - cfg.data()));
        if (c.amd_run || c.fmd_run || (c.agc_run && c.agc_mode != 0) || c.lms[0].run || c.lms[1].run || c.amsq_run || c.emnr_run || c.snba_run || c.ap_on() || c.ssql_on()) k.mixed = true;
        if (c.ssql_on() && ((int)(0.070 * dsp_rate) < 64))
            return set_error(QH_ERR_UNSUPPORTED, "SSQL needs ramps of 64 samples or more: dsp_rate %d is too low", dsp_rate);
        if (c.emnr_run && !emnr_tables) return set_error(QH_ERR_INVALID, "EMNR needs its gain tables first (qh_rxa_SetEMNRTables: WDSP's `calculus` and `zetaHat.bin` data)");
        if (c.nbp_run) { k.any_nbp = true; if (c.nbp_nc > k.nc_max) k.nc_max = c.nbp_nc; } else k.every_nbp = false;
        if (c.bp1_run) { k.any_bp1 = true; if (c.bp1_nc > k.nc_max) k.nc_max = c.bp1_nc; }
        if (c.fmd_run && c.fm_nc > k.nc_max) k.nc_max = c.fm_nc;
    }
    if (k.nc_max > kLongNcMax) return set_error(QH_ERR_UNSUPPORTED, "nc = %d exceeds %d", k.nc_max, kLongNcMax);
    return QH_OK;
}

// stages whose impulse response is longer than 4096 taps run in partitions (run_band): how many, per stage
int Engine::plan_long(ChainCall &k)
{
    auto parts = [](int nc) { return nc > kLongPart ? (nc + kLongPart - 1) / kLongPart : 1; };
    int lp[5] = { 1, 1, 1, 1, 1 };
    // Over every channel that runs the stage OR still holds a long delay line of it: a fircore keeps its delay line while it does not run (xbandpass / xnbp with run = 0
    // only copy; SetRXABandpassRun, a mode change back to AM / FM, RXANBPSetRun switch it on again without a flush), so a channel with
    // nc > 4096 that sits out holds 16383 samples the one-tile form has no room for.  Had the form followed the RUNNING channels,
    // the only long channel leaving took the stage to the short form (its line cut to 4095 samples) and came back to zeros behind
    // them: one long call 0.65 off (walk rxa_long 900190, found by round 6's seed sweep; in the suite since).
    // (long_live: the channel has run the stage with such an nc since RXASetNC last zeroed its lines.)
    for (ChanCfg &c : cfg) {
        const int pn = parts(c.nbp_nc), pb = parts(c.bp1_nc), pf = parts(c.fm_nc);
        if (c.nbp_run && pn > 1) c.long_live[0] = true;
        if (c.bp1_run && pb > 1) c.long_live[1] = true;
        if (c.fmd_run && pf > 1) c.long_live[2] = true;
        if (c.snba_run && pn > 1) c.long_live[4] = true;
        if (c.nbp_run || c.long_live[0]) lp[0] = std::max(lp[0], pn);
        if (c.bp1_run || c.long_live[1]) lp[1] = std::max(lp[1], pb);
        if (c.fmd_run || c.long_live[2]) lp[2] = lp[3] = std::max(lp[2], pf);
        if (c.snba_run || c.long_live[4]) lp[4] = std::max(lp[4], pn);
    }
    for (int sid = 0; sid < 5; sid++) {
        if (lp[sid] > 1) { k.long_mode = true; if (int rc = long_stage_alloc(sid, sid == 2 || sid == 3)) return rc; }
        if (lp[sid] == long_parts[sid]) continue;
        if (int rc = quiesce()) return rc;
        if ((lp[sid] > 1) != (long_parts[sid] > 1)) {       // the delay lines move with the form
            double2 **hs = sid == 0 ? hist_nbp : sid == 1 ? hist_bp1 : sid == 2 ? hist_de : sid == 3 ? hist_aud : hist_snb;
            // BOTH ping-pong halves: a channel that has left the stage's list (another mode, bp1 or SNBA switched off) keeps its rows in
            // the half that was current when it left (bp1_hist_at, fm_hist_at, snb_hist_at), which need not be the current one
            for (int half = 0; half < 2; half++)
                if (hs[half] && lhist[sid][half])
                    hipLaunchKernelGGL(long_migrate_kernel, dim3(16, (unsigned)nch), dim3(NT), 0, stream, hs[half], lhist[sid][half], lp[sid] > 1 ? 1 : 0);
        }
        long_parts[sid] = lp[sid];
        for (ChanCfg &c : cfg) {            // the stage's masks are laid out for another form now: all of them again
            if (sid == 0) c.nbp_dirty = true;
            if (sid == 1) c.bp1_dirty = true;
            if (sid == 4) c.snb_dirty = true;
        }
        if (sid == 2 || sid == 3) fm_nc_built = 0;
    }
    return QH_OK;
}

// The fircore tile.  Impulse responses longer than 2048 taps need 8192 points (osfir_kernel<8192>, one wave per SIMD).
// Shorter ones run 4096-point tiles; the two-group 8192-point tile (osfir8k_kernel, 6144 instead of 2049 outputs per
// pair of transforms) is there on request (qh_rxa_set_band_tile) -- it measured slower, see qh_osfir.hpp.  The masks are
// spectra of the tile size, so a change rebuilds every one of them (the delay lines, kept 4095 samples deep, carry over).
void Engine::pick_band_tile(int nc_max)
{
    const bool two_group = nc_max <= 2048 && band_tile_pref == 8192;
    const bool six_k = nc_max <= 2048 && band_tile_pref == 6144;
    const int want = six_k ? kOsfir6kN : (nc_max > 2048 || two_group) ? kBandNfftMax : kNfft;
    if (want != bnfft || two_group != band2g || six_k != band6k) {
        bnfft = want; band2g = two_group; band6k = six_k;
        for (ChanCfg &c : cfg) { c.nbp_dirty = c.bp1_dirty = true; c.snb_dirty = true; }
    }
}

// xrxa (wdsp/RXA.c:560-597) for every channel: the linear chains' fast path, or the per-mode stages on channel lists
int Engine::process_chain(const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk)
{
    if (nblk <= 0) return QH_OK;
    QH_HIP(hipSetDevice(device));
    ChainCall k;
    k.nblk = nblk;
    if (int rc = chain_needs(k)) return rc;
    if (int rc = plan_long(k)) return rc;
    pick_band_tile(k.nc_max);
    // The three meters of xrxa (adc, S, agc: RXA.c:566,569,589) ride on the nbp0 launch when the chain is linear (nbp0 runs,
    // bp1 does not, fixed AGC gain): the band tile then starts on a multiple of 256 samples so that a register holds one
    // 64-sample chunk per wavefront.  Any other chain takes the per-mode path with the stand-alone meter kernel.
    k.meters_fused = meters_on && !k.mixed && k.any_nbp && !k.any_bp1 && dsp_size >= 64 && dsp_size <= 2048 && !k.long_mode;
    if (meters_on && !k.meters_fused) k.mixed = true;
    if (meters_on) if (int rc = meters_alloc()) return rc;
    if (int rc = refresh_params()) return rc;
    if (k.mixed) if (int rc = refresh_demod()) return rc;
    if (lists[L_SNBA].n) if (int rc = refresh_params()) return rc;       // bpsnba's mask needs the buffers the line above may just have made

    k.n_in = (long long)nblk * dsp_insize;
    k.n_mid = (long long)nblk * dsp_size;
    if (k.n_in > 0x7fffffffLL) return set_error(QH_ERR_INVALID, "too many samples in one call");
    if (int rc = ensure_buffers(k.n_mid)) return rc;
    if (k.long_mode) if (int rc = long_buffers()) return rc;
    if (int rc = refresh_ap(k)) return rc;
    if (int rc = refresh_ssql(k)) return rc;
    ev_used = 0;

    k.in = reinterpret_cast<const double2 *>(d_in); k.in_stride = in_stride;
    k.out = reinterpret_cast<double2 *>(d_out); k.out_stride = out_stride;
    // (with a partitioned stage in the call the others run 4096-tap tiles: their own nc is at most that)
    k.P = band6k ? kOsfir6kP : band2g ? kOsfir8kP : k.meters_fused ? ((k.nc_max - 1 + 255) / 256) * 256 : k.long_mode ? kLongPart - 1 : k.nc_max - 1;
    // audio egress (qh_rxa_process_audio): the narrowing rides in the store of the last kernel when that is an overlap-save
    // band stage or the per-mode path's output pass; other endings write complex doubles to the staging rows and narrow after
    k.eg_fused = eg.kind && (k.mixed ? lists[L_AMSQ].n == 0 : ((k.any_nbp || k.any_bp1) && !k.long_mode));
    if (eg.kind && !k.eg_fused) {
        if (int rc = ensure_abuf(k.n_mid)) return rc;
        k.out = abuf; k.out_stride = abuf_cap;
    }
    if (!k.mixed) return run_linear(k);

    // ---- mixed modes: per-mode stages run on channel lists; gains / panel in a final pointwise pass
    if (int rc = plan_mixed(k)) return rc;
    if (int rc = run_mixed_front(k)) return rc;     // xshift, xresample, adc meter, xnbp, S meter, xamsqcap, xbpsnbaout 0
    if (int rc = run_am(k)) return rc;              // xamd's AM / SAM channels (and their bp1 when it ends their chain)
    if (k.side) QH_HIP(hipEventRecord(ev_join, side_stream));
    if (lists[L_FM].n) if (int rc = run_fm(k)) return rc;    // xfmd
    if (k.side) QH_HIP(hipStreamWaitEvent(stream, ev_join, 0));
    if (lists[L_SNB + 1].n) snb_inplace(k, lists[L_SNB + 1].dev, lists[L_SNB + 1].n);       // xbpsnbain / xbpsnbaout at position 1 (RXA.c:576-577)
    if (lists[L_SNB].n || lists[L_SNB + 1].n) cur_snb ^= 1;
    if (int rc = run_snba(k)) return rc;            // xsnba, RXA.c:578
    // xanf, xanr, xbandpass(bp1) at position 0, xwcpagc, then the same three at position 1 (RXA.c:579-586).  The two bp1
    // launches work on disjoint channel rows of one ping-pong history pair, so the pair flips once for both.
    lms_at(k, 0, k.cur);
    bp1_at(k, 0);
    // xwcpagc modes 1-4 (sequential per channel); mode 0 rides in the output matrix below unless a position-1 stage follows
    tick(1);
    if (lists[L_AGC_CUR].n || lists[L_AGC_OTHER].n) if (int rc = run_agc(k)) return rc;
    run_output(k);                                  // position 1, agc meter, xwcpagc mode 0 + xpanel, xamsq, egress
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// ---- every channel is a linear chain: the epilogue rides on the last stage, no extra pass
int Engine::run_linear(ChainCall &k)
{
    const long long n_mid = k.n_mid;
    const int nstage = 1 + (k.any_nbp ? 1 : 0) + (k.any_bp1 ? 1 : 0);
    int stage = 0, which = 0;
    const double2 *cur = k.in;
    long long cur_stride = k.in_stride;
    auto dst_of = [&](int st, long long &stride) -> double2 * {
        if (st == nstage - 1) { stride = k.out_stride; return k.out; }
        stride = buf_cap;
        double2 *p = buf[which];
        which ^= 1;
        return p;
    };
    {
        long long dst_stride;
        double2 *dst = dst_of(stage, dst_stride);
        // A chain that is the front stage alone stores to the caller's rows while other tiles -- and the history pass behind the kernel --
        // still read the input: when the rows of the two matrices overlap (include/quiskhip.h: the output may lie over the input) the
        // stage goes to the engine's own rows and the output is written in a last pass.
        const bool over = nstage == 1 && !extents_apart(k.out, k.out_stride, n_mid, k.in, k.in_stride, k.n_in, nch);
        if (over) { dst = buf[0]; dst_stride = buf_cap; }
        if (int rc = run_front(cur, cur_stride, dst, dst_stride, stage == nstage - 1 ? epi : nullptr, k.n_in, n_mid)) return rc;
        if (over) QH_HIP(hipMemcpy2DAsync(k.out, (size_t)k.out_stride * sizeof(double2), dst, (size_t)dst_stride * sizeof(double2),
                                          (size_t)n_mid * sizeof(double2), (size_t)nch, hipMemcpyDeviceToDevice, stream));
        cur = dst; cur_stride = dst_stride; stage++;
    }
    for (int f = 0; f < 2; f++) {
        if (f == 0 ? !k.any_nbp : !k.any_bp1) continue;
        long long dst_stride;
        double2 *dst = dst_of(stage, dst_stride);
        if (k.meters_fused) if (int rc = ensure_meter_partials(n_mid, bnfft - k.P)) return rc;
        run_band(cur, cur_stride, dst, dst_stride, stage == nstage - 1 ? epi : nullptr, n_mid,
                 f == 0 ? mask_nbp : mask_bp1, kBandNfftMax, f == 0 ? hist_nbp : hist_bp1, f == 0 ? cur_nbp : cur_bp1, k.P,
                 nullptr, 0, k.meters_fused, k.eg_fused && stage == nstage - 1);
        cur = dst; cur_stride = dst_stride; stage++;
    }
    if (k.meters_fused)
        hipLaunchKernelGGL(meter_finish_kernel, dim3((unsigned)nch), dim3(kMeterFinishThreads), 0, stream, m_part[0], m_part[1],
                           m_part_cap, (int)(n_mid / 64), dsp_size / 64, (bnfft - k.P) / 64, band6k ? 2 : band2g ? 1 : 0, m_adc, m_s, m_agc,
                           -1.0 / ((double)dsp_rate * 0.100), -1.0 / ((double)dsp_rate * 0.100), (const double *)m_g2);
    if (eg.kind && !k.eg_fused) pack_audio(k.out, k.out_stride, n_mid);
    tick(3);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// The forms of the per-mode path's stages, and the buffers they need
int Engine::plan_mixed(ChainCall &k)
{
    // FM channels have a long detector chain of kernels that fill a fraction of the chip (one lane per 256-sample tile of the loop,
    // a few workgroups per channel in the scans) while the other channels' work is dense filtering.  With both kinds in the call
    // the FM channels' front and nbp0 stages are launched first and their detector chain follows on the main stream; the other
    // channels' front, nbp0 and AM detectors run beside it on a second stream (fork / join by events, which a launch-sequence
    // capture records as graph edges).  BASELINE config 4: 1.20 -> 0.8 ms per call.
    // dbg_forms (QH_DBG_FORMS in the environment when the engine is made; diagnostics: tools/dbg/determinism_stress2.py and the failure
    // branch of tests/test_gpu_properties_fullsize.py): bit 0 no second stream for the filters, 1 no stores straight to the caller's rows,
    // 2 no envelope in nbp0's store, 3 no angles in nbp0's store, 4 no paired real filters, 5 no second stream at all, 6-7 where the second
    // stream forks (counted down from behind the FM channels' nbp0), 8 xfmd's dc removal as a pass of its own (fm_dc_tiled_kernel), 9 the AM
    // fade leveller as a pass of its own (am_level_tiled_kernel)
    k.split = lists[L_FM].n > 0 && lists[L_REST].n > 0 && D > 1 && !meters_on && !lists[L_AMSQ].n && !lists[L_SNB].n && !timing && !(dbg_forms & 1);
    // ... and when nothing sits between a channel's last filter and the output matrix (no AGC state machine, LMS, EMNR, SNBA,
    // limiter, squelch or position-1 stage anywhere), that last stage -- nbp0 for the plain channels, bp1 for AM / SAM, the CTCSS
    // notch for FM -- applies the matrix in its store and writes the caller's buffer: the output pass (32 B per output sample) goes.
    k.fm_theta_fused = k.split && k.any_nbp && !band6k && !band2g && bnfft == kNfft && !(dbg_forms & 8);
    bool no_lms = true;
    for (int f = 0; f < 2; f++) for (int p = 0; p < 3; p++) no_lms = no_lms && !lists[L_LMS + 3 * f + p].n;
    k.direct = k.split && !(dbg_forms & 2) && k.every_nbp && !eg.kind && !lists[L_LIM].n && !lists[L_AGC_CUR].n && !lists[L_AGC_OTHER].n && !lists[L_SNBA].n && !lists[L_SNB + 1].n && no_lms &&
               !lists[L_EMNR].n && !lists[L_EMNR + 1].n && !lists[L_EMNR + 2].n && !lists[L_FIX].n && !lists[L_FIX + 1].n && !lists[L_BP1P + 1].n && lists[L_BP1P].n == lists[L_BP1].n && lists[L_RB].n == lists[L_BP1].n &&
               lists[L_USB].n + lists[L_FM].n == lists[L_PLAIN].n && !lists[L_AP].n && !lists[L_AP + 1].n && !ssql_listed() &&
               // the first stores to `out` come while other channels' input is still being read: not for a caller that works in place
               extents_apart(k.out, k.out_stride, k.n_mid, k.in, k.in_stride, k.n_in, nch);
    // ... and the AM channels' nbp0 leaves the envelope and every tile's share of the fade leveller's averages: one pass does the rest
    k.P_am = ((k.P + 63) / 64) * 64;
    k.am_fused = k.direct && !(dbg_forms & 4) && lists[L_AM].n > 0 && lists[L_RB].n == lists[L_AM].n + lists[L_SAM].n && !band6k && !band2g && bnfft == kNfft && k.P_am < bnfft;
    // ... or, when the tiles are 2048 outputs behind 2048 samples of pre-roll and bp1 takes its channels two a tile, no pass at all: the
    // leveller's local share in nbp0's store (DET 3), the carried share in bp1's load
    k.am_lv_fused = k.am_fused && k.P_am == 2048 && bnfft - k.P_am == 2048 && np_am > 0 && lists[L_BP1P].n && long_parts[1] <= 1 && !(dbg_forms & (16 | 512));
    // The AM / SAM detectors and the FM detector chain touch disjoint channel rows and disjoint state, and neither fills the
    // chip (one workgroup or wavefront per channel): with both kinds of channel in the call the AM side runs on a second
    // stream, forked and joined by events (which a launch-sequence capture records as graph edges).
    k.side = k.split || ((lists[L_AM].n || lists[L_SAM].n) && lists[L_FM].n && !(dbg_forms & 32));
    if (k.am_fused) {
        if (int rc = grow(am_tsum, am_tsum_cap, (k.n_mid + (bnfft - k.P_am) - 1) / (bnfft - k.P_am), 2LL * nch)) return rc;
        if (k.am_lv_fused) if (int rc = grow(am_cin, am_cin_cap, am_tsum_cap + 1, 2LL * nch)) return rc;
    }
    if (k.side) if (int rc = ensure_side_stream()) return rc;
    for (double *&q : seg_sum)
        if (!q) if (int rc = alloc(q, (long long)nch * kSegWaves * kSegMaxGroups * kSegSumW)) return rc;
    k.cur = buf[0]; k.other = buf[1];
    return QH_OK;
}

int Engine::ensure_side_stream()
{
    if (side_stream) return QH_OK;
    QH_HIP(hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking));
    QH_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    QH_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    return QH_OK;
}

// what the second stream runs from here on follows what the main stream has launched so far
int Engine::fork_side()
{
    QH_HIP(hipEventRecord(ev_fork, stream));
    QH_HIP(hipStreamWaitEvent(side_stream, ev_fork, 0));
    return QH_OK;
}

// The per-mode path's front and nbp0 stages, split over the two streams or not, the adc and S meters, xamsqcap and xbpsnbaout at
// position 0
int Engine::run_mixed_front(ChainCall &k)
{
    const long long n_in = k.n_in, n_mid = k.n_mid;
    const int P = k.P;
    double2 *&cur = k.cur, *&other = k.other;
    if (k.split) {
        if (int rc = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid, nullptr, 0, 1)) return rc;      // tile table, every channel
        // Where the second stream starts: behind the FM channels' nbp0 (2; the default), behind their front (1) or at once (0) -- QH_DBG_FORMS
        // bits 6-7 count DOWN from 2 (experiments).  The FM channels' chain is the longer one and ends in kernels that cannot fill the chip
        // (the loop's lanes, the CTCSS notch's scans): with their front and nbp0 alone on the chip first, all of them run beside the other
        // channels' dense filters (config 4, one box: 10.45 ms forked at once, 10.31 forked here).
        const int fork_at = 2 - (((dbg_forms >> 6) & 3) > 2 ? 2 : ((dbg_forms >> 6) & 3));
        if (fork_at == 0) if (int rc = fork_side()) return rc;
        if (int rc = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid, lists[L_FM].dev, lists[L_FM].n, 2)) return rc;
        if (fork_at == 1) if (int rc = fork_side()) return rc;
        int hc = cur_nbp;
        // the FM channels' nbp0 feeds the loop's phase detector and nothing else: its store takes the angles (first half of the rows)
        if (k.any_nbp) run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, mask_nbp, kBandNfftMax, hist_nbp, hc, P, lists[L_FM].dev, lists[L_FM].n, false, false,
                                k.fm_theta_fused ? 1 : 0, reinterpret_cast<double *>(other), 2 * buf_cap);
        if (fork_at >= 2) if (int rc = fork_side()) return rc;
        std::swap(stream, side_stream);
        int rc2 = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid, lists[L_REST].dev, lists[L_REST].n, 2);
        hc = cur_nbp;
        if (!rc2 && k.any_nbp) {
            if (k.direct) {     // the plain channels end here: output matrix in the store, straight to the caller's buffer
                if (lists[L_USB].n) run_band(cur, buf_cap, k.out, k.out_stride, epi, n_mid, mask_nbp, kBandNfftMax, hist_nbp, hc, P, lists[L_USB].dev, lists[L_USB].n);
                hc = cur_nbp;
                if (k.am_fused) {
                    if (lists[L_SAM].n) run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, mask_nbp, kBandNfftMax, hist_nbp, hc, P, lists[L_SAM].dev, lists[L_SAM].n);
                    hc = cur_nbp;
                    run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, mask_nbp, kBandNfftMax, hist_nbp, hc, k.P_am, lists[L_AM].dev, lists[L_AM].n, false, false,
                             k.am_lv_fused ? 3 : 2, reinterpret_cast<double *>(other), 2 * buf_cap);
                } else if (lists[L_RB].n) run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, mask_nbp, kBandNfftMax, hist_nbp, hc, P, lists[L_RB].dev, lists[L_RB].n);
            } else run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, mask_nbp, kBandNfftMax, hist_nbp, hc, P, lists[L_REST].dev, lists[L_REST].n);
        }
        std::swap(stream, side_stream);
        if (rc2) return rc2;
        if (k.any_nbp) { cur_nbp ^= 1; std::swap(cur, other); }
        if (int rc = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid, nullptr, 0, 3)) return rc;          // histories, oscillator phases
    } else {
        if (int rc = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid)) return rc;
        if (meters_on) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)nch), dim3(64), 0, stream, cur, buf_cap, k.nblk, dsp_size, m_adc,
                                          m_prm, (const int *)nullptr);
        if (k.any_nbp) {
            run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, mask_nbp, kBandNfftMax, hist_nbp, cur_nbp, P, nullptr, 0);
            std::swap(cur, other);
        }
    }
    if (meters_on) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)nch), dim3(64), 0, stream, cur, buf_cap, k.nblk, dsp_size, m_s,
                                      m_prm, (const int *)nullptr);
    if (lists[L_AMSQ].n) {           // xamsqcap (RXA.c:571): the magnitudes of the signal behind nbp0, for xamsq at the end of the chain
        if (int rc = grow(amsq_mag, amsq_mag_cap, buf_cap, nch)) return rc;
        long long per = (n_mid + NT - 1) / NT;
        hipLaunchKernelGGL(amsq_cap_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)lists[L_AMSQ].n), dim3(NT), 0, stream, cur, buf_cap,
                           (int)n_mid, lists[L_AMSQ].dev, amsq_mag, amsq_mag_cap);
    }
    // xbpsnbaout at position 0 (RXA.c:572): the 250..5700 Hz filter of the signal ahead of nbp0 replaces nbp0's output
    if (lists[L_SNB].n) {
        if (k.any_nbp) { int hc = cur_snb; run_band(other, buf_cap, cur, buf_cap, nullptr, n_mid, mask_snb, kBandNfftMax, hist_snb, hc, P, lists[L_SNB].dev, lists[L_SNB].n); }
        else snb_inplace(k, lists[L_SNB].dev, lists[L_SNB].n);
    }
    tick(1);
    return QH_OK;
}

// bpsnba on the listed channels' rows of cur, through the rows of other
void Engine::snb_inplace(const ChainCall &k, const int *list, int n)
{
    int hc = cur_snb;
    run_band(k.cur, buf_cap, k.other, buf_cap, nullptr, k.n_mid, mask_snb, kBandNfftMax, hist_snb, hc, k.P, list, n);
    long long per = (k.n_mid + NT - 1) / NT;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)n), dim3(NT), 0, stream, k.other, k.cur, buf_cap,
                       (int)k.n_mid, list);
}

// Segment scans: one 16-wavefront workgroup per channel fills one CU.  With fewer channels of a kind than the chip has CUs the
// call is cut into 16 G segments, G workgroups per channel, pass 1 and pass 2 as two launches (qh_wave.hpp, MODE 1 / 2).
int Engine::seg_groups(int count, long long n_mid) const
{
    int G = count > 0 ? 256 / count : 1;
    while (G > 1 && n_mid / (64LL * kSegWaves * G) < 8) G--;        // at least 8 batches of 64 samples per segment
    return G < 1 ? 1 : G > kSegMaxGroups ? kSegMaxGroups : G;
}

// xamd's envelope and fade leveller over the listed channels' rows of cur in G segments (SAM: mixed with the phases pts):
// pass 1, pass 2 and the commit of the carried states, or one pass
template <bool SAM>
void Engine::am_detect(const ChainCall &k, hipStream_t s, const int *list, int n, int G, const double *pts, long long pts_stride, double *gs)
{
    if (G > 1) {
        hipLaunchKernelGGL((am_detect_tiled_kernel<SAM, 1>), dim3((unsigned)n, (unsigned)G), dim3(kSegThreads), 0, s, k.cur, buf_cap,
                           (int)k.n_mid, list, levelfade, am_state, am_prm, pts, pts_stride, gs);
        hipLaunchKernelGGL((am_detect_tiled_kernel<SAM, 2>), dim3((unsigned)n, (unsigned)G), dim3(kSegThreads), 0, s, k.cur, buf_cap,
                           (int)k.n_mid, list, levelfade, am_state, am_prm, pts, pts_stride, gs, am_next);
        hipLaunchKernelGGL(commit_am_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, am_state, (const AmState *)am_next, list, n, levelfade);
    } else
        hipLaunchKernelGGL((am_detect_tiled_kernel<SAM, 0>), dim3((unsigned)n), dim3(kSegThreads), 0, s, k.cur, buf_cap, (int)k.n_mid,
                           list, levelfade, am_state, am_prm, pts, pts_stride, (double *)nullptr);
}

// xamd for the AM and SAM channels, on the second stream when the call has FM channels too; and bp1 behind them there when it is
// their last stage
int Engine::run_am(ChainCall &k)
{
    const long long n_mid = k.n_mid;
    double2 *cur = k.cur, *other = k.other;
    hipStream_t am_stream = stream;
    if (k.split) am_stream = side_stream;         // forked already: the AM detectors follow the other channels' filters there
    else if (k.side) {
        if (int rc = fork_side()) return rc;
        am_stream = side_stream;
    }
    FmDcSrc amlv_src{ nullptr, 0, 0 };
    if (lists[L_AM].n && k.am_lv_fused) {    // the envelope + the leveller's local share lie in the channels' own rows (first half); bp1 loads them from there
        hipLaunchKernelGGL(am_lv_chain_kernel, dim3((unsigned)lists[L_AM].n), dim3(64), 0, am_stream, (int)n_mid, bnfft - k.P_am, lists[L_AM].dev, (const int *)levelfade, am_state,
                           am_prm, (const double *)am_tsum, am_tsum_cap, (const double *)am_last, am_cin, am_cin_cap);
        amlv_src = FmDcSrc{ reinterpret_cast<double *>(cur), 2 * buf_cap, 11 };
    } else if (lists[L_AM].n && k.am_fused) {  // envelopes in the channels' own rows (first half), audio to the rows of `other`
        const int G = seg_groups(lists[L_AM].n + (n_mid >= kSamTiledMin ? n_sam0 : 0), n_mid);
        hipLaunchKernelGGL(am_level_tiled_kernel, dim3((unsigned)lists[L_AM].n, (unsigned)G), dim3(kSegThreads), 0, am_stream,
                           (const double *)reinterpret_cast<double *>(cur), 2 * buf_cap, other, buf_cap, (int)n_mid, lists[L_AM].dev, levelfade, (const AmState *)am_state,
                           am_prm, (const double *)am_tsum, am_tsum_cap, bnfft - k.P_am, am_next);
        hipLaunchKernelGGL(commit_am_kernel, dim3((unsigned)((lists[L_AM].n + 255) / 256)), dim3(256), 0, am_stream, am_state, (const AmState *)am_next, lists[L_AM].dev, lists[L_AM].n, levelfade);
    } else if (lists[L_AM].n)
        am_detect<false>(k, am_stream, lists[L_AM].dev, lists[L_AM].n, seg_groups(lists[L_AM].n + (n_mid >= kSamTiledMin ? n_sam0 : 0), n_mid), nullptr, 0, seg_sum[0]);
    {
        // SAM without sideband separation in a long call: angles, the loop one tile per lane with a warm-up, verify / repair,
        // then the mix with the phase each sample saw and the fade leveller over time segments (qh_tiled.hpp).  The channels'
        // rows of `other` are free here: first half = angles, second half = phases.  Short calls and the all-pass modes
        // (SAM-L / SAM-U) take the sequential kernel.
        // (the channels with a sideband selected follow the others in lists[L_SAM].dev: the loop is the same, the chains come behind it)
        const int nt = n_mid >= kSamTiledMin ? lists[L_SAM].n : 0, nt0 = nt ? n_sam0 : 0, ntsb = nt - nt0;
        if (nt) {
            double *theta = reinterpret_cast<double *>(other), *pts = theta + buf_cap;
            const long long per = (n_mid + NT - 1) / NT;
            hipLaunchKernelGGL(pll_theta_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)nt), dim3(NT), 0, am_stream, cur, buf_cap,
                               (int)n_mid, lists[L_SAM].dev, theta, 2 * buf_cap);
            const long long ntl = (n_mid + kSamTile - 1) / kSamTile;
            const int ngroups = (int)((ntl + 63) / 64);
            if (int rc = grow(pll_ends, pll_ends_cap, (long long)ngroups * 64, (long long)nch * kPllEndsW)) return rc;
            hipLaunchKernelGGL((pll_lanes_kernel<true>), dim3((unsigned)ngroups, (unsigned)nt), dim3(64), 0, am_stream, (const double *)theta,
                               2 * buf_cap, pts, 2 * buf_cap, (int)n_mid, lists[L_SAM].dev, (const PllState *)pll_state, pll_ends, pll_ends_cap * kPllEndsW,
                               sam_pll_prm, kSamTile, kSamWarm);
            hipLaunchKernelGGL((pll_verify_kernel<true>), dim3((unsigned)nt), dim3(64), 0, am_stream, (const double *)theta, 2 * buf_cap, pts,
                               2 * buf_cap, (int)n_mid, lists[L_SAM].dev, pll_state, pll_ends, pll_ends_cap * kPllEndsW, sam_pll_prm, kSamTile, kSamWarm,
                               pll_nfixed, pll_check_only);
            if (nt0)        // (the segment summaries behind the AM channels' rows)
                am_detect<true>(k, am_stream, lists[L_SAM].dev, nt0, seg_groups(lists[L_AM].n + nt, n_mid), pts, 2 * buf_cap,
                                seg_sum[0] + (size_t)lists[L_AM].n * kSegWaves * kSegMaxGroups * kSegSumW);
            if (ntsb) {
                const int G = seg_groups(lists[L_AM].n + nt, n_mid), S = kSegWaves * G;
                if (int rc = set_sb_phi(n_mid, S)) return rc;
                const int *lst = lists[L_SAM].dev + nt0;
                double *gs = seg_sum[0] + (size_t)(lists[L_AM].n + nt0) * kSegWaves * kSegMaxGroups * kSegSumW;
                hipLaunchKernelGGL((sam_sb_tiled_kernel<1>), dim3((unsigned)ntsb, (unsigned)(S / kSbWaves)), dim3(64 * kSbWaves), 0, am_stream, cur, buf_cap, (int)n_mid,
                                   lst, (const SamChanParam *)sam_prm, (const double *)pts, 2 * buf_cap, pll_state, sb_sum, (const double *)sb_start);
                hipLaunchKernelGGL(sam_sb_chain_kernel, dim3((unsigned)ntsb), dim3(64), 0, am_stream, (int)n_mid, S, lst, (const PllState *)pll_state,
                                   (const double *)sb_phi, (const double *)sb_sum, sb_start);
                hipLaunchKernelGGL((sam_sb_tiled_kernel<2>), dim3((unsigned)ntsb, (unsigned)(S / kSbWaves)), dim3(64 * kSbWaves), 0, am_stream, cur, buf_cap, (int)n_mid,
                                   lst, (const SamChanParam *)sam_prm, (const double *)pts, 2 * buf_cap, pll_state, sb_sum, (const double *)sb_start);
                hipLaunchKernelGGL((sam_level_tiled_kernel<1>), dim3((unsigned)ntsb, (unsigned)G), dim3(kSegThreads), 0, am_stream, cur, buf_cap, (int)n_mid,
                                   lst, levelfade, (const AmState *)am_state, am_prm, gs, am_next);
                hipLaunchKernelGGL((sam_level_tiled_kernel<2>), dim3((unsigned)ntsb, (unsigned)G), dim3(kSegThreads), 0, am_stream, cur, buf_cap, (int)n_mid,
                                   lst, levelfade, (const AmState *)am_state, am_prm, gs, am_next);
                hipLaunchKernelGGL(commit_am_kernel, dim3((unsigned)((ntsb + 255) / 256)), dim3(256), 0, am_stream, am_state, (const AmState *)am_next, lst, ntsb, levelfade);
            }
        }
        if (lists[L_SAM].n - nt) hipLaunchKernelGGL(sam_pll_kernel, dim3((unsigned)(lists[L_SAM].n - nt)), dim3(64), 0, am_stream, cur, buf_cap, (int)n_mid,
                                           lists[L_SAM].dev + nt, pll_state, sam_prm, sam_pll_prm, am_state);
    }
    if (k.direct && lists[L_BP1P].n) {      // bp1 is the AM / SAM channels' last stage: it follows their detectors on the second stream
        std::swap(stream, side_stream);
        int hc = cur_bp1;
        if (k.am_fused) {
            if (amlv_src.a) band_amlv = &amlv_src;
            run_band(other, buf_cap, k.out, k.out_stride, epi, n_mid, mask_bp1, kBandNfftMax, hist_bp1, hc, k.P, lists[L_AM].dev, lists[L_AM].n, false, false, 0, nullptr, 0,
                     np_am && !(dbg_forms & 16) ? lists[L_PAIRS_AM].dev : nullptr, np_am);
            band_amlv = nullptr;
            hc = cur_bp1;
            if (lists[L_SAM].n) run_band(cur, buf_cap, k.out, k.out_stride, epi, n_mid, mask_bp1, kBandNfftMax, hist_bp1, hc, k.P, lists[L_SAM].dev, lists[L_SAM].n, false, false, 0,
                                nullptr, 0, np_sam && !(dbg_forms & 16) ? lists[L_PAIRS_SAM].dev : nullptr, np_sam);
        } else run_band(cur, buf_cap, k.out, k.out_stride, epi, n_mid, mask_bp1, kBandNfftMax, hist_bp1, hc, k.P, lists[L_BP1P].dev, lists[L_BP1P].n);
        std::swap(stream, side_stream);
    }
    return QH_OK;
}

// xfmd (fmd.c): the loop, dc removal and gain, de-emphasis, audio filter, CTCSS notch and the detector limiter
int Engine::run_fm(ChainCall &k)
{
    const long long n_mid = k.n_mid;
    double2 *cur = k.cur, *other = k.other;
    // xfmd's loop (fmd.c:151-172), time-tiled (qh_tiled.hpp): angles, then one loop per lane and tile, then dc removal + gain.
    // The FM channels' rows of `other` are free here: first half = angles, second half = loop filter output.
    const bool pair = de_real && np_fm && !band6k && !band2g && bnfft == kNfft && !(dbg_forms & 16);      // the de-emphasis stage two channels a tile
    // fmdc_fused: the dc removal and gain (fmd.c:169-171) do not get a pass of their own -- the loop kernels take the tile's own
    // share of the average off (local_dc), a chain over the tiles' contributions gives the average ahead of every tile, and the
    // de-emphasis stage's load takes the rest off and applies the gain (OsfirArgs::fmdc_*): 8 bytes per sample read there instead
    // of 8 read + 16 written here and 16 read there
    const bool fmdc_fused = pair && long_parts[2] <= 1 && !(dbg_forms & 256);
    FmDcSrc fmdc_src{ nullptr, 0, 0 };
    {
        // fused: nbp0 left the angles in the channels' own rows (first half) and the loop output goes to the rows of `other`
        double *theta = reinterpret_cast<double *>(k.fm_theta_fused ? cur : other), *fil = reinterpret_cast<double *>(other) + buf_cap;
        if (fmdc_fused) fil = reinterpret_cast<double *>(cur) + buf_cap;     // (the de-emphasis stage reads it while it writes the rows of `other`)
        const long long per = (n_mid + NT - 1) / NT;
        if (!k.fm_theta_fused)
            hipLaunchKernelGGL(pll_theta_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)lists[L_FM].n), dim3(NT), 0, stream, cur, buf_cap,
                               (int)n_mid, lists[L_FM].dev, theta, 2 * buf_cap);
        // the longest tile that still gives the chip 512 wavefronts of 64 tiles: the 768-sample warm-up is 3/4 of a 256-sample
        // tile's steps and 3/11 of a 2048-sample tile's
        int fm_tile = kFmTile;
        while (fm_tile < 2048 && (long long)lists[L_FM].n * n_mid / (64LL * 2 * fm_tile) >= 512) fm_tile *= 2;
        const long long ntl = (n_mid + fm_tile - 1) / fm_tile;
        const int ngroups = (int)((ntl + 63) / 64);
        if (int rc = grow(pll_ends, pll_ends_cap, (long long)ngroups * 64, (long long)nch * kPllEndsW)) return rc;
        if (fmdc_fused) if (int rc = grow(fm_cin, fm_cin_cap, pll_ends_cap + 1, nch)) return rc;
        hipLaunchKernelGGL((pll_lanes_kernel<false>), dim3((unsigned)ngroups, (unsigned)lists[L_FM].n), dim3(64), 0, stream, (const double *)theta,
                           2 * buf_cap, fil, 2 * buf_cap, (int)n_mid, lists[L_FM].dev, (const PllState *)fm_pll_state, pll_ends, pll_ends_cap * kPllEndsW,
                           fm_pll_prm, fm_tile, kFmWarm, fmdc_fused ? 1 : 0);
        hipLaunchKernelGGL((pll_verify_kernel<false>), dim3((unsigned)lists[L_FM].n), dim3(64), 0, stream, (const double *)theta, 2 * buf_cap, fil,
                           2 * buf_cap, (int)n_mid, lists[L_FM].dev, fm_pll_state, pll_ends, pll_ends_cap * kPllEndsW, fm_pll_prm, fm_tile, kFmWarm,
                           pll_nfixed, pll_check_only, fmdc_fused ? 1 : 0);
        if (fmdc_fused) {
            hipLaunchKernelGGL(fm_dc_chain_kernel, dim3((unsigned)lists[L_FM].n), dim3(64), 0, stream, (int)n_mid, fm_tile, lists[L_FM].dev, fm_pll_state, fm_pll_prm,
                               (const double *)pll_ends, pll_ends_cap * kPllEndsW, fm_cin, fm_cin_cap);
            int sh = 0;
            while ((1 << sh) < fm_tile) sh++;
            fmdc_src = FmDcSrc{ fil, 2 * buf_cap, sh };
        } else {
            // dc removal + gain: the tiles' contributions are in `ends` already, one pass over `fil`
            const int G = seg_groups(lists[L_FM].n, n_mid);
            hipLaunchKernelGGL(fm_dc_tiled_kernel, dim3((unsigned)lists[L_FM].n, (unsigned)G), dim3(kSegThreads), 0, stream, (const double *)fil,
                               2 * buf_cap, cur, buf_cap, (int)n_mid, lists[L_FM].dev, (const PllState *)fm_pll_state, (const double *)fm_again, fm_pll_prm,
                               (const double *)pll_ends, pll_ends_cap * kPllEndsW, fm_tile, fmdc_next);
            hipLaunchKernelGGL(commit_fmdc_kernel, dim3((unsigned)((lists[L_FM].n + 255) / 256)), dim3(256), 0, stream, fm_pll_state, (const double *)fmdc_next, lists[L_FM].dev, lists[L_FM].n);
        }
    }
    {   // de-emphasis: real taps on a real signal, two channels per tile
        if (fmdc_src.a) band_fmdc = &fmdc_src;
        run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, mask_de, 0, hist_de, cur_de, k.P, lists[L_FM].dev, lists[L_FM].n, false, false, 0, nullptr, 0,
                 pair ? lists[L_PAIRS_FM].dev : nullptr, np_fm);
        band_fmdc = nullptr;
    }
    run_band(other, buf_cap, cur, buf_cap, nullptr, n_mid, mask_aud, 0, hist_aud, cur_aud, k.P, lists[L_FM].dev, lists[L_FM].n);   // audio filter
    tick(1);
    {
        const int G = seg_groups(lists[L_FM].n, n_mid);
        if (G > 1) {
            hipLaunchKernelGGL((snotch_tiled_kernel<1>), dim3((unsigned)lists[L_FM].n, (unsigned)G), dim3(kSegThreads), 0, stream, cur, buf_cap, (int)n_mid,
                               lists[L_FM].dev, sn_prm, sn_state, seg_sum[2]);
            hipLaunchKernelGGL((snotch_tiled_kernel<2>), dim3((unsigned)lists[L_FM].n, (unsigned)G), dim3(kSegThreads), 0, stream, cur, buf_cap, (int)n_mid,
                               lists[L_FM].dev, sn_prm, sn_state, seg_sum[2], k.direct ? k.out : (double2 *)nullptr, k.out_stride, (const EpiParam *)epi, sn_next);
            hipLaunchKernelGGL(commit_snotch_kernel, dim3((unsigned)((lists[L_FM].n + 255) / 256)), dim3(256), 0, stream, sn_state, (const SnotchState *)sn_next, lists[L_FM].dev, lists[L_FM].n,
                               (const SnotchParam *)sn_prm);
        } else
            hipLaunchKernelGGL((snotch_tiled_kernel<0>), dim3((unsigned)lists[L_FM].n), dim3(kSegThreads), 0, stream, cur, buf_cap, (int)n_mid, lists[L_FM].dev,
                               sn_prm, sn_state, (double *)nullptr, k.direct ? k.out : (double2 *)nullptr, k.out_stride, (const EpiParam *)epi);
    }
    if (lists[L_LIM].n)      // detector limiter: lim_pre_gain 0.4, then its own wcpAGC (fmd.c:179-184)
        hipLaunchKernelGGL(agc_form == 1 ? wcpagc_seq_kernel : wcpagc_kernel, dim3((unsigned)lists[L_LIM].n), dim3(64), 0, stream, cur, buf_cap,
                           (int)n_mid, lists[L_LIM].dev, lim_prm, lim_state, 0.4);
    return QH_OK;
}

// xsnba, with the tuning the setters left uploaded first
int Engine::run_snba(const ChainCall &k)
{
    if (!lists[L_SNBA].n) return QH_OK;
    if (snba_tune_dirty) {
        QH_HIP(hipMemcpyAsync(snba_tune, snba_tune_h.data(), snba_tune_h.size() * sizeof(SnbaTune), hipMemcpyHostToDevice, stream));
        QH_HIP(hipStreamSynchronize(stream));
        snba_tune_dirty = false;
    }
    hipLaunchKernelGGL(snba_kernel, dim3((unsigned)lists[L_SNBA].n), dim3(64), 0, stream, k.cur, buf_cap, k.nblk, dsp_size, lists[L_SNBA].dev, snba_prm,
                       snba_hin, snba_hout, snba_state, snba_idx, snba_scratch, (const SnbaTune *)snba_tune);
    return QH_OK;
}

// xanf and xanr of list entry pos ([f][0] position 0; [f][1 + b] position 1 with the data in cur / other), on the rows of b, and
// xemnr behind them (RXA.c:581,585)
void Engine::lms_at(const ChainCall &k, int pos, double2 *b)
{
    for (int f = 0; f < 2; f++)
        if (lists[L_LMS + 3 * f + pos].n) hipLaunchKernelGGL(lms_kernel, dim3((unsigned)lists[L_LMS + 3 * f + pos].n), dim3(64), 0, stream, b, buf_cap, (int)k.n_mid,
                                              lists[L_LMS + 3 * f + pos].dev, lms_prm[f], lms_state[f]);
    if (lists[L_EMNR + pos].n)
        hipLaunchKernelGGL(emnr_kernel, dim3((unsigned)lists[L_EMNR + pos].n), dim3(NT), (size_t)emnr_lds_bytes(), stream, b, buf_cap, k.nblk, lists[L_EMNR + pos].dev,
                           emnr_prm, emnr_chan, emnr_scal, emnr_state, emnr_window, tw4096, emnr_GG, emnr_GGS, emnr_zeta, emnr_zeta_true);
}

// xbandpass (bp1) at position pos, from the rows of cur to those of other -- unless bp1 ended the AM / SAM channels' chain already
void Engine::bp1_at(const ChainCall &k, int pos)
{
    int hc = cur_bp1;
    if (lists[L_BP1P + pos].n && !k.direct)
        run_band(k.cur, buf_cap, k.other, buf_cap, nullptr, k.n_mid, mask_bp1, kBandNfftMax, hist_bp1, hc, k.P, lists[L_BP1P + pos].dev, lists[L_BP1P + pos].n);
}

// xwcpagc modes 1-4.  Long calls: the level detector in time tiles, everything around it lane-parallel (qh_agc_tiled.hpp).  Short
// calls (the drop-in's blocks), a channel whose attack window moved in mid-stream, and the diagnostic forms: one wavefront per channel.
int Engine::run_agc(ChainCall &k)
{
    const long long n_mid = k.n_mid;
    double2 *cur = k.cur, *other = k.other;
    bool tiled = (agc_form == 0 || agc_form == 3) && n_mid >= kAgcTiledMin;      // (3: diagnostics, the tiles' check counts and repairs nothing)
    int a_max = 0;
    for (int ch = 0; ch < nch && tiled; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (!c.agc_on() || c.agc_stale) continue;
        a_max = c.agc_abuf > a_max ? c.agc_abuf : a_max;
    }
    // the tiles take the channels at the head of each list, the stepping kernel the ones behind them (all of them in a short call)
    const int nt_cur = tiled ? lists[L_AGC_CUR].n - n_agc_cur_stale : 0, nt_other = tiled ? lists[L_AGC_OTHER].n - n_agc_other_stale : 0;
    if (nt_cur + nt_other == 0) tiled = false;
    agc_last_tiled = nt_cur + nt_other;
    for (ChanCfg &c : cfg) if (c.agc_on()) c.agc_ran = true;
    // the reference's full ring (RB_SIZE entries): this call's last inputs go in where xwcpagc writes them; a channel whose attack
    // window moved since its last call first takes its 2048-entry ring again from it (the entries the longer window jumped over)
    if (!agc_lring) {
        if (int rc = quiesce()) return rc;
        if (int rc = alloc(agc_lring, (long long)nch * kAgcLongRing, true)) return rc;
        if (int rc = alloc(agc_labs, (long long)nch * kAgcLongRing, true)) return rc;
        if (int rc = alloc(agc_lout, nch)) return rc;
        if (int rc = alloc(agc_rewin_list, nch)) return rc;
        QH_HIP(hipMemsetAsync(agc_lout, 0xff, (size_t)nch * sizeof(int), stream));          // out_index = -1 (calc_wcpagc, wcpAGC.c:34)
    }
    {
        std::vector<int> rw;
        for (int ch = 0; ch < nch; ch++) {
            ChanCfg &c = cfg[(size_t)ch];
            if (c.agc_on() && c.agc_rewindow) rw.push_back(ch);
            if (c.agc_on()) c.agc_rewindow = false;
        }
        if (!rw.empty()) {
            QH_HIP(hipMemcpyAsync(agc_rewin_list, rw.data(), rw.size() * sizeof(int), hipMemcpyHostToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
            hipLaunchKernelGGL(agc_rewindow_kernel, dim3((unsigned)rw.size()), dim3(256), 0, stream, (const int *)agc_rewin_list, agc_state,
                               (const double2 *)agc_lring, (const double *)agc_labs, (const int *)agc_lout);
        }
    }
    {
        const long long span = n_mid < kAgcLongRing ? n_mid : kAgcLongRing;
        const unsigned gx = (unsigned)((span + 255) / 256 < 120 ? (span + 255) / 256 : 120);
        auto mirror = [&](const double2 *b, const int *lst, int cnt) {
            if (!cnt) return;
            hipLaunchKernelGGL(agc_long_mirror_kernel, dim3(gx, (unsigned)cnt), dim3(256), 0, stream, b, buf_cap, (int)n_mid, lst, (const AgcParam *)agc_prm,
                               agc_lring, agc_labs, (const int *)agc_lout);
            hipLaunchKernelGGL(agc_long_advance_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, (int)n_mid, lst, cnt, agc_lout);
        };
        mirror(cur, lists[L_AGC_CUR].dev, lists[L_AGC_CUR].n);
        mirror(other, lists[L_AGC_OTHER].dev, lists[L_AGC_OTHER].n);
    }
    // ... and when every channel has the AGC as its last stage (nothing at position 1, no meters, squelch or audio frames), the gain
    // multiply applies the output matrix and writes the caller's rows: the output pass goes
    bool no_p1 = !lists[L_BP1P + 1].n && !lists[L_FIX].n && !lists[L_FIX + 1].n && !lists[L_EMNR + 1].n && !lists[L_EMNR + 2].n && !lists[L_AMSQ].n && !meters_on && !eg.kind && !lists[L_AP].n && !lists[L_AP + 1].n &&
                 !ssql_listed();
    for (int f = 0; f < 2; f++) for (int p = 1; p < 3; p++) no_p1 = no_p1 && !lists[L_LMS + 3 * f + p].n;
    k.agc_direct = tiled && no_p1 && nt_cur == lists[L_PLAIN].n && nt_other == lists[L_BP1].n;
    if (tiled) {
        const int nl = nt_cur > nt_other ? nt_cur : nt_other;
        const int ntile = (int)((n_mid + kAgcTile - 1) / kAgcTile), hp = (a_max + 15) & ~15;
        // tiles short enough for one to two wavefronts of 64 tiles per SIMD
        int L = 256;
        while (L < 16384 && (long long)nl * n_mid / (64LL * 2 * L) >= 1024) L *= 2;
        const long long nt_l = (n_mid + L - 1) / L, ngroups = (nt_l + 63) / 64;
        if (n_mid > agc_arr || ngroups * 64 > agc_ends_cap || (long long)ntile * hp > agc_halo_cap) {
            if (int rc = quiesce()) return rc;
            const long long arr = std::max(n_mid, agc_arr), ends = std::max(ngroups * 64, agc_ends_cap), halo = std::max((long long)ntile * hp, agc_halo_cap);
            auto tiles = [](long long n) { return (n + kAgcTile - 1) / kAgcTile; };
            if (int rc = alloc(agc_scr, nch * 4 * arr)) return rc;
            if (int rc = alloc(agc_ends, nch * ends * kAgcEndsW * 2)) return rc;    // boundary states, then end states
            if (int rc = alloc(agc_halo, nch * halo)) return rc;
            if (int rc = alloc(agc_tsum, nch * tiles(arr) * 2)) return rc;
            agc_arr = arr; agc_ends_cap = ends; agc_halo_cap = halo;
            if (!agc_fin) {
                if (int rc = alloc(agc_fin, nch * 8)) return rc;
                if (int rc = alloc(agc_tail, (long long)nch * kAgcRing)) return rc;
                if (int rc = alloc(agc_nfixed, 2, true)) return rc;
                if (int rc = alloc(agc_sege, 2LL * nch * kAgcSegs * 8)) return rc;    // two copies: a repair round reads one and writes the other
            }
        }
        static bool agc_attr = false;
        if (!agc_attr) {        // attack windows of up to kAgcRing samples: more dynamic LDS than the default limit
            QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(agc_prep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       3 * (kAgcRing + kAgcTile) * (int)sizeof(double)));
            QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(agc_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (kAgcRing + kAgcTile) * (int)sizeof(double2)));
            agc_attr = true;
        }
        auto run = [&](double2 *b, const int *lst, int cnt) {
            if (!cnt) return;
            const int n = (int)n_mid;
            const int G = seg_groups(cnt, n_mid);
            const size_t lds_prep = (size_t)3 * (((size_t)a_max + 63) / 64 * 64 + kAgcTile) * sizeof(double);
            const size_t lds_apply = ((size_t)a_max + kAgcTile) * sizeof(double2);
            hipLaunchKernelGGL(agc_prep_kernel, dim3((unsigned)ntile, (unsigned)cnt), dim3(256), lds_prep, stream, (const double2 *)b, buf_cap, n,
                               lst, (const AgcParam *)agc_prm, (const AgcState *)agc_state, agc_scr, agc_arr, agc_halo, hp, 1.0, agc_tsum);
            hipLaunchKernelGGL(agc_avg_tiled_kernel, dim3((unsigned)cnt, (unsigned)G), dim3(kSegThreads), 0, stream, (const double2 *)b,
                               buf_cap, n, lst, (const AgcParam *)agc_prm, (const AgcState *)agc_state, agc_scr, agc_arr, (const double *)agc_tsum,
                               ntile, 1.0);
            double *bnd = agc_ends, *end = agc_ends + (size_t)nch * (size_t)agc_ends_cap * kAgcEndsW;
            // the boundary pass over K super-segments per channel at once (a multiple of the tile length each)
            int K = 1;
            while (K < kAgcSegs && (long long)cnt * K < 4096 && n_mid / (2 * K) >= 8 * L && n_mid / (2 * K) >= 32768) K *= 2;
            if (const char *e = getenv("QH_AGC_SEGS")) { const int v = atoi(e); if (v >= 1 && v <= kAgcSegs) K = v; }
            const int seg = (int)(((n_mid + K - 1) / K + L - 1) / L) * L;
            // No warm-up ahead of a segment by default: every segment starts from the state the call began in, and the repair rounds
            // walk each one again from the end of the one before it until the two walks meet (agc_bounds_round_kernel) -- the work a
            // warm-up long enough for every channel (400 attack windows on the bench input) spends on all of them, spent only where
            // and for as long as the walks differ.
            int wmul = 0, rounds = 3;
            if (const char *e = getenv("QH_AGC_WARM")) { const int v = atoi(e); if (v >= 0) wmul = v; }
            if (const char *e = getenv("QH_AGC_ROUNDS")) { const int v = atoi(e); if (v >= 0 && v <= 16) rounds = v; }
            const int Wm = ((wmul * a_max + L - 1) / L) * L;
            double *sg[2] = { agc_sege, agc_sege + (size_t)nch * kAgcSegs * 8 };
            hipLaunchKernelGGL(agc_bounds_kernel, dim3((unsigned)cnt, (unsigned)K), dim3(64), 0, stream, n, lst, (const AgcParam *)agc_prm,
                               (const AgcState *)agc_state, (const double *)agc_scr, agc_arr, bnd, agc_ends_cap * kAgcEndsW, L, seg, Wm, sg[0]);
            if (K > 1) {
                int at = 0;
                for (int r = 0; r < rounds; r++, at ^= 1)
                    hipLaunchKernelGGL(agc_bounds_round_kernel, dim3((unsigned)cnt, (unsigned)K), dim3(64), 0, stream, n, lst,
                                       (const AgcParam *)agc_prm, (const double *)agc_scr, agc_arr, bnd, agc_ends_cap * kAgcEndsW, L, seg, K,
                                       (const double *)sg[at], sg[at ^ 1], agc_nfixed + 1);
                hipLaunchKernelGGL(agc_bounds_fix_kernel, dim3((unsigned)cnt), dim3(64), 0, stream, n, lst, (const AgcParam *)agc_prm,
                                   (const double *)agc_scr, agc_arr, bnd, agc_ends_cap * kAgcEndsW, L, seg, K, sg[at], agc_nfixed + 1);
            }
            hipLaunchKernelGGL(agc_lanes_kernel, dim3((unsigned)ngroups, (unsigned)cnt), dim3(64), 0, stream, n, lst, (const AgcParam *)agc_prm,
                               agc_scr, agc_arr, (const double *)bnd, agc_ends_cap * kAgcEndsW, end, agc_ends_cap * kAgcEndsW, L);
            hipLaunchKernelGGL(agc_verify_kernel, dim3((unsigned)cnt), dim3(64), 0, stream, n, lst, (const AgcParam *)agc_prm, agc_scr, agc_arr,
                               (const double *)bnd, agc_ends_cap * kAgcEndsW, end, agc_ends_cap * kAgcEndsW, L, agc_fin, agc_nfixed, agc_form == 3 ? 1 : 0);
            hipLaunchKernelGGL(agc_tail_kernel, dim3((unsigned)cnt), dim3(256), 0, stream, (const double2 *)b, buf_cap, n, lst,
                               (const AgcParam *)agc_prm, agc_tail, 1.0);
            hipLaunchKernelGGL(agc_apply_kernel, dim3((unsigned)ntile, (unsigned)cnt), dim3(256), lds_apply, stream, b, buf_cap, n, lst,
                               (const AgcParam *)agc_prm, (const double *)agc_scr, agc_arr, (const double2 *)agc_halo, hp, 1.0,
                               k.agc_direct ? k.out : (double2 *)nullptr, k.out_stride, (const EpiParam *)epi);
            hipLaunchKernelGGL(agc_finish_kernel, dim3((unsigned)cnt), dim3(256), 0, stream, n, lst, (const AgcParam *)agc_prm, agc_state,
                               (const double *)agc_scr, agc_arr, (const double2 *)agc_tail, (const double *)agc_fin);
        };
        run(cur, lists[L_AGC_CUR].dev, nt_cur);
        run(other, lists[L_AGC_OTHER].dev, nt_other);
    }
    if (const int ns = lists[L_AGC_CUR].n - nt_cur)
        hipLaunchKernelGGL(agc_form == 1 ? wcpagc_seq_kernel : wcpagc_kernel, dim3((unsigned)ns), dim3(64), 0, stream, cur, buf_cap, (int)n_mid,
                           (const int *)(lists[L_AGC_CUR].dev + nt_cur), agc_prm, agc_state, 1.0);
    if (const int ns = lists[L_AGC_OTHER].n - nt_other)
        hipLaunchKernelGGL(agc_form == 1 ? wcpagc_seq_kernel : wcpagc_kernel, dim3((unsigned)ns), dim3(64), 0, stream, other, buf_cap, (int)n_mid,
                           (const int *)(lists[L_AGC_OTHER].dev + nt_other), agc_prm, agc_state, 1.0);
    return QH_OK;
}

// ---- xcbl, xspeak, xmpeak (qh_audio_peak.hpp)
int Engine::ap_alloc()
{
    if (int rc = alloc(ap_prm, nch)) return rc;
    if (int rc = alloc(ap_state, (long long)nch * kApW, true)) return rc;
    if (int rc = alloc(ap_M, (long long)nch * kApDim * kApDim)) return rc;
    ap_M_h.assign((size_t)nch * kApDim * kApDim, 0.0);
    ap_prm_h.assign((size_t)nch, ApParam{});
    ap_L = 0;
    for (ChanCfg &c : cfg) { c.ap_dirty = true; c.sp_flush = false; for (bool &f : c.mp_flush) f = false; }    // the state starts at zero
    return QH_OK;
}

// T = A^L: A's column i is where one step with zero input takes the unit state e_i (ap_step_linear, the kernel's own recurrence);
// powers by squaring.  Stages that do not run leave their rows at the identity.
static void ap_transition(const ApParam &q, int L, double *T)
{
    constexpr int N = kApDim;
    std::vector<double> A((size_t)N * N), R((size_t)N * N, 0.0), tmp((size_t)N * N);
    for (int i = 0; i < N; i++) {
        double s[N] = {};
        s[i] = 1.0;
        (void)ap_step_linear(q, s, 0.0);
        for (int r = 0; r < N; r++) A[(size_t)r * N + i] = s[r];
    }
    for (int i = 0; i < N; i++) R[(size_t)i * N + i] = 1.0;
    auto mul = [&](const std::vector<double> &X, const std::vector<double> &Y, std::vector<double> &Z) {
        for (int r = 0; r < N; r++)
            for (int c = 0; c < N; c++) {
                long double acc = 0.0L;
                for (int k = 0; k < N; k++) acc += (long double)X[(size_t)r * N + k] * Y[(size_t)k * N + c];
                Z[(size_t)r * N + c] = (double)acc;
            }
    };
    for (int e = L; e > 0; e >>= 1) {
        if (e & 1) { mul(R, A, tmp); R.swap(tmp); }
        if (e > 1) { mul(A, A, tmp); A.swap(tmp); }
    }
    std::copy(R.begin(), R.end(), T);
}

// Parameters, carry matrices and flushes of the three stages, and the tile length of this call (before anything is enqueued)
int Engine::refresh_ap(const ChainCall &k)
{
    if (!ap_prm) {
        for (ChanCfg &c : cfg) { c.sp_flush = false; for (bool &f : c.mp_flush) f = false; }
        return QH_OK;
    }
    const int nap = k.mixed ? lists[L_AP].n + lists[L_AP + 1].n : 0;
    int L = ap_L;
    if (nap) {
        // tiles short enough for about four wavefronts of 64 tiles per SIMD (1024 SIMDs), 256 .. 8192 samples
        L = 256;
        while (L < 8192 && (long long)nap * k.n_mid / L > 4LL * 64 * 1024) L *= 2;
        const long long ntile = (k.n_mid + L - 1) / L;
        if (int rc = grow(ap_ends, ap_ends_cap, ntile, (long long)kApW * nch)) return rc;
    }
    const double mtau = std::exp(-1.0 / ((double)dsp_rate * 0.02));       // calc_cbl, cblock.c:29-36 (tau 0.02, RXA.c:411)
    auto bq = [&](double f, double bw, double g) {
        const SpeakDesign d = design_speak(f, bw, g, (double)dsp_rate);
        return ApBiquad{ d.a0, d.a1, d.a2, d.b1, d.b2, d.fgain };
    };
    bool up = false;
    const ApParam *last_q = nullptr;
    const double *last_T = nullptr;
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (c.sp_flush || c.mp_flush[0] || c.mp_flush[1]) {            // flush_speak: that cascade's x / y history, I and Q
            for (int comp = 0; comp < 2; comp++) {
                double *st = ap_state + (size_t)ch * kApW + (size_t)comp * kApDim;
                if (c.sp_flush) QH_HIP(hipMemsetAsync(st + kApSpeakAt, 0, kApCascade * sizeof(double), stream));
                for (int p = 0; p < kApPeaks; p++)
                    if (c.mp_flush[p]) QH_HIP(hipMemsetAsync(st + kApPeakAt + kApCascade * p, 0, kApCascade * sizeof(double), stream));
            }
            c.sp_flush = false;
            for (bool &f : c.mp_flush) f = false;
        }
        if (!c.ap_dirty && !(nap && L != ap_L && c.ap_on())) continue;
        ApParam &q = ap_prm_h[(size_t)ch];
        q = ApParam{};
        q.sp = bq(c.sp_f, c.sp_bw, c.sp_gain);
        for (int p = 0; p < kApPeaks; p++) q.pk[p] = bq(c.mp_f[p], c.mp_bw[p], c.mp_gain[p]);
        q.mtau = mtau;
        q.flags = (c.cbl_run ? AP_CBL : 0) | (c.sp_run ? AP_SPEAK : 0) | (c.mp_run ? AP_MPEAK : 0);
        for (int p = 0; p < kApPeaks; p++)
            if (c.mp_run && c.mp_enable[p] && p < c.mp_npeaks) q.flags |= AP_PEAK0 << p;
        double *T = ap_M_h.data() + (size_t)ch * kApDim * kApDim;
        if (c.ap_on() && nap) {
            if (last_q && std::memcmp(last_q, &q, sizeof(q)) == 0) std::copy(last_T, last_T + kApDim * kApDim, T);
            else ap_transition(q, L, T);
            last_q = &q; last_T = T;
            QH_HIP(hipMemcpyAsync(ap_M + (size_t)ch * kApDim * kApDim, T, (size_t)kApDim * kApDim * sizeof(double), hipMemcpyHostToDevice, stream));
        }
        QH_HIP(hipMemcpyAsync(ap_prm + ch, &q, sizeof(q), hipMemcpyHostToDevice, stream));
        c.ap_dirty = false;
        up = true;
    }
    if (up) QH_HIP(hipStreamSynchronize(stream));
    ap_L = L;
    return QH_OK;
}

// the three stages of the listed channels, in place on the rows that hold them behind bp1 (cur / other)
void Engine::run_audio_peak(const ChainCall &k)
{
    if (!ap_prm || (!lists[L_AP].n && !lists[L_AP + 1].n)) return;
    const int n = (int)k.n_mid, L = ap_L;
    const long long ntile = (k.n_mid + L - 1) / L, estride = ap_ends_cap * kApW;
    const unsigned ngroups = (unsigned)((ntile + 63) / 64);
    for (int b = 0; b < 2; b++) {
        if (!lists[L_AP + b].n) continue;
        double2 *rows = b ? k.other : k.cur;
        if (ntile > 1)
            hipLaunchKernelGGL(audio_peak_pass_kernel<0>, dim3(ngroups, (unsigned)lists[L_AP + b].n), dim3(64), 0, stream, rows, buf_cap, n,
                               (const int *)lists[L_AP + b].dev, (const ApParam *)ap_prm, ap_state, ap_ends, estride, L);
        hipLaunchKernelGGL(audio_peak_carry_kernel, dim3((unsigned)lists[L_AP + b].n), dim3(64), 0, stream, n, L, (const int *)lists[L_AP + b].dev,
                           (const double *)ap_M, (const double *)ap_state, ap_ends, estride);
        hipLaunchKernelGGL(audio_peak_pass_kernel<1>, dim3(ngroups, (unsigned)lists[L_AP + b].n), dim3(64), 0, stream, rows, buf_cap, n,
                           (const int *)lists[L_AP + b].dev, (const ApParam *)ap_prm, ap_state, ap_ends, estride, L);
    }
}

// ---- xssql (qh_ssql.hpp)
int Engine::ssql_alloc()
{
    const double rate = (double)dsp_rate;
    if (int rc = alloc(ssql_list_block, 2LL * nch)) return rc;
    for (int b = 0; b < 2; b++) ssql_lists[b].dev = ssql_list_block + (size_t)nch * b;
    if (int rc = alloc(ssql_prm, nch)) return rc;
    if (int rc = alloc(ssql_state, nch)) return rc;
    SsqlState z{};                                  // calc_ssql (ssql.c:133-140): all zero but the trigger voltage, MUTED
    z.v = kSsTrThresh; z.state = SS_MUTED; z.count = 0;
    std::vector<SsqlState> st((size_t)nch, z);
    QH_HIP(hipMemcpyAsync(ssql_state, st.data(), st.size() * sizeof(SsqlState), hipMemcpyHostToDevice, stream));
    // compute_ssql_slews (ssql.c:110-127), muted_gain 0, tup = tdown = 0.070 (RXA.c:452-454): theta accumulates as there
    const double mg = 0.0;
    ssql_ntup = (int)(0.070 * rate); ssql_ntdown = (int)(0.070 * rate);
    std::vector<double> up((size_t)ssql_ntup + 1), down((size_t)ssql_ntdown + 1);
    double delta = kPiRef / (double)ssql_ntup, theta = 0.0;
    for (int i = 0; i <= ssql_ntup; i++) { up[(size_t)i] = mg + (1.0 - mg) * 0.5 * (1.0 - std::cos(theta)); theta += delta; }
    delta = kPiRef / (double)ssql_ntdown; theta = 0.0;
    for (int i = 0; i <= ssql_ntdown; i++) { down[(size_t)i] = mg + (1.0 - mg) * 0.5 * (1.0 + std::cos(theta)); theta += delta; }
    if (int rc = alloc(ssql_cup, (long long)up.size())) return rc;
    if (int rc = alloc(ssql_cdown, (long long)down.size())) return rc;
    QH_HIP(hipMemcpyAsync(ssql_cup, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(ssql_cdown, down.data(), down.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));
    ssql_prm_h.assign((size_t)nch, SsqlParam{});
    ssql_L = 0;
    for (ChanCfg &c : cfg) c.ssql_dirty = true;
    return QH_OK;
}

// A^L for a D x D transition A (row-major), by squaring in long double
static void ssql_power(const double *A0, int D, int L, double *T)
{
    std::vector<long double> A(A0, A0 + D * D), R((size_t)D * D, 0.0L), tmp((size_t)D * D);
    for (int i = 0; i < D; i++) R[(size_t)i * D + i] = 1.0L;
    auto mul = [&](const std::vector<long double> &X, const std::vector<long double> &Y, std::vector<long double> &Z) {
        for (int r = 0; r < D; r++)
            for (int c = 0; c < D; c++) {
                long double acc = 0.0L;
                for (int k = 0; k < D; k++) acc += X[(size_t)r * D + k] * Y[(size_t)k * D + c];
                Z[(size_t)r * D + c] = acc;
            }
    };
    for (int e = L; e > 0; e >>= 1) {
        if (e & 1) { mul(R, A, tmp); R.swap(tmp); }
        if (e > 1) { mul(A, A, tmp); A.swap(tmp); }
    }
    for (int i = 0; i < D * D; i++) T[i] = (double)R[(size_t)i];
}

// Parameters and carry transitions of the listed channels, and the tile length of this call (before anything is enqueued)
int Engine::refresh_ssql(const ChainCall &k)
{
    if (!ssql_prm) return QH_OK;
    const int nss = k.mixed ? ssql_lists[0].n + ssql_lists[1].n : 0;
    int L = ssql_L;
    if (nss) {
        // as the audio-peak stages: about four wavefronts of 64 tiles per SIMD, 256 .. 8192 samples (a multiple of 64: whole words)
        L = 256;
        while (L < 8192 && (long long)nss * k.n_mid / L > 4LL * 64 * 1024) L *= 2;
        const long long ntile = (k.n_mid + L - 1) / L, nw = kSsHistW + (k.n_mid + 63) / 64 + 1;
        if (int rc = grow(ssql_ends, ssql_ends_cap, ntile, (long long)kSsE * nch)) return rc;
        if (int rc = grow(ssql_bits, ssql_wcap, nw, 3LL * nch)) return rc;
        if (int rc = grow(ssql_rec, ssql_rec_cap, nw, (long long)nch)) return rc;      // grows with ssql_wcap: the same stride
    }
    const double rate = (double)dsp_rate;
    SsqlParam base{};
    base.mtau = std::exp(-1.0 / (rate * 0.02));                         // calc_cbl, cblock.c:35 (create_cbl of calc_ssql, tau 0.02)
    base.div = 2000.0 * 2.0 * kSsRing / rate;                          // create_ftov, ssql.c:51 (fmax 2000, rsize 2400)
    {                                                                   // calc_dbqlp, iir.c:829-843: fc 11.3, Q 1.0
        const double w0 = kTwoPiRef * 11.3 / rate, cs = std::cos(w0), c = std::sin(w0) / (2.0 * 1.0), den = 1.0 + c;
        base.a0 = 0.5 * (1.0 - cs) / den; base.a1 = (1.0 - cs) / den; base.a2 = 0.5 * (1.0 - cs) / den;
        base.b1 = 2.0 * cs / den; base.b2 = (c - 1.0) / den;
    }
    base.wdmult = std::exp(-1.0 / (rate * 0.5));                        // calc_ssql, ssql.c:136 (wdtau 0.5)
    base.muted_gain = 0.0;
    base.ntup = ssql_ntup; base.ntdown = ssql_ntdown;
    if (nss) {
        const double Ac[4] = { 0.0, 0.0, -1.0, base.mtau };             // (xp, y) -> (0, -xp + mtau y)
        const double om = 1.0 - base.wdmult;                            // (y1, y2, w) -> (y0, y1, wdmult w + (1 - wdmult) y0)
        const double Al[9] = { base.b1, base.b2, 0.0, 1.0, 0.0, 0.0, om * base.b1, om * base.b2, base.wdmult };
        ssql_power(Ac, 2, L, base.Tc);
        ssql_power(Al, 3, L, base.Tl);
    }
    bool up = false;
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (!c.ssql_dirty && !(nss && L != ssql_L && c.ssql_on())) continue;
        SsqlParam &q = ssql_prm_h[(size_t)ch];
        q = base;
        q.wthresh = c.ssql_wthresh;
        q.mute_mult = 1.0 - std::exp(-1.0 / (rate * c.ssql_tau_mute));            // ssql.c:137-138, :339-370
        q.unmute_mult = 1.0 - std::exp(-1.0 / (rate * c.ssql_tau_unmute));
        QH_HIP(hipMemcpyAsync(ssql_prm + ch, &q, sizeof(q), hipMemcpyHostToDevice, stream));
        c.ssql_dirty = false;
        up = true;
    }
    if (up) QH_HIP(hipStreamSynchronize(stream));
    if (nss) ssql_L = L;
    return QH_OK;
}

// the squelch of the listed channels, in place on the rows that hold them behind bp1 (cur / other)
void Engine::run_ssql(const ChainCall &k)
{
    if (!ssql_prm || !ssql_listed()) return;
    const int n = (int)k.n_mid, L = ssql_L;
    const long long ntile = (k.n_mid + L - 1) / L, estride = ssql_ends_cap * kSsE, ws = ssql_wcap;
    unsigned long long *xb = ssql_bits, *wdb = xb + (size_t)nch * ws, *trb = wdb + (size_t)nch * ws;
    const unsigned ngroups = (unsigned)((ntile + 63) / 64);
    const long long per = (k.n_mid + 255) / 256;
    const unsigned gx = (unsigned)(per < 1024 ? per : 1024);
    for (int b = 0; b < 2; b++) {
        const int nl = ssql_lists[b].n;
        if (!nl) continue;
        double2 *rows = b ? k.other : k.cur;
        const int *lst = ssql_lists[b].dev;
        const dim3 tiles(ngroups, (unsigned)nl);
        if (ntile > 1)
            hipLaunchKernelGGL(ssql_cbl_kernel<0>, tiles, dim3(64), 0, stream, (const double2 *)rows, buf_cap, n, lst, (const SsqlParam *)ssql_prm,
                               ssql_state, ssql_ends, estride, xb, ws, L);
        hipLaunchKernelGGL((ssql_carry_kernel<2, false>), dim3((unsigned)nl), dim3(64), 0, stream, n, L, lst, (const SsqlParam *)ssql_prm,
                           (const SsqlState *)ssql_state, ssql_ends, estride);
        hipLaunchKernelGGL(ssql_cbl_kernel<1>, tiles, dim3(64), 0, stream, (const double2 *)rows, buf_cap, n, lst, (const SsqlParam *)ssql_prm,
                           ssql_state, ssql_ends, estride, xb, ws, L);
        if (ntile > 1)
            hipLaunchKernelGGL(ssql_lp_kernel<0>, tiles, dim3(64), 0, stream, n, lst, (const SsqlParam *)ssql_prm, ssql_state, ssql_ends, estride,
                               (const unsigned long long *)xb, wdb, ws, L);
        hipLaunchKernelGGL((ssql_carry_kernel<3, false>), dim3((unsigned)nl), dim3(64), 0, stream, n, L, lst, (const SsqlParam *)ssql_prm,
                           (const SsqlState *)ssql_state, ssql_ends, estride);
        hipLaunchKernelGGL(ssql_lp_kernel<1>, tiles, dim3(64), 0, stream, n, lst, (const SsqlParam *)ssql_prm, ssql_state, ssql_ends, estride,
                           (const unsigned long long *)xb, wdb, ws, L);
        hipLaunchKernelGGL((ssql_carry_kernel<1, true>), dim3((unsigned)nl), dim3(64), 0, stream, n, L, lst, (const SsqlParam *)ssql_prm,
                           (const SsqlState *)ssql_state, ssql_ends, estride);
        hipLaunchKernelGGL(ssql_trigger_kernel, tiles, dim3(64), 0, stream, n, lst, (const SsqlParam *)ssql_prm, ssql_state,
                           (const double *)ssql_ends, estride, (const unsigned long long *)wdb, trb, ws, L);
        hipLaunchKernelGGL(ssql_walk_kernel, dim3((unsigned)nl), dim3(64), 0, stream, n, lst, (const SsqlParam *)ssql_prm, ssql_state,
                           (const unsigned long long *)trb, ssql_rec, (const unsigned long long *)xb, ws);
        hipLaunchKernelGGL(ssql_apply_kernel, dim3(gx, (unsigned)nl), dim3(256), 0, stream, rows, buf_cap, n, lst, (const SsqlParam *)ssql_prm,
                           (const unsigned long long *)trb, (const int *)ssql_rec, ws, (const double *)ssql_cup, (const double *)ssql_cdown);
    }
}

// xwcpagc mode 0 where a position-1 stage follows it, xanf / xanr / xemnr / bp1 at position 1, the agc meter, then xwcpagc mode 0 +
// xpanel in the output pass, xamsq and the audio frames
void Engine::run_output(const ChainCall &k)
{
    const long long n_mid = k.n_mid, per = (n_mid + NT - 1) / NT;
    const unsigned gx = (unsigned)(per < 1024 ? per : 1024);
    for (int b = 0; b < 2; b++)
        if (lists[L_FIX + b].n) hipLaunchKernelGGL(scale_kernel, dim3(gx, (unsigned)lists[L_FIX + b].n), dim3(NT), 0, stream, b ? k.other : k.cur, buf_cap,
                                         (int)n_mid, lists[L_FIX + b].dev, fix_gain);
    lms_at(k, 1, k.cur);
    lms_at(k, 2, k.other);
    bp1_at(k, 1);
    if (lists[L_BP1].n) cur_bp1 ^= 1;
    if (meters_on) {    // agcmeter sits after xwcpagc (RXA.c:589); mode 0's gain multiply is applied below, so its
                        // level reading is taken on the fixed-gain input times g^2 (m_g2)
        if (lists[L_PLAIN].n) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)lists[L_PLAIN].n), dim3(64), 0, stream, k.cur, buf_cap, k.nblk, dsp_size,
                                        m_agc, m_prm, lists[L_PLAIN].dev, (const double *)m_g2);
        if (lists[L_BP1].n) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)lists[L_BP1].n), dim3(64), 0, stream, k.other, buf_cap, k.nblk, dsp_size,
                                      m_agc, m_prm, lists[L_BP1].dev, (const double *)m_g2);
    }
    run_audio_peak(k);                  // xcbl, xspeak, xmpeak (RXA.c:591-593)
    run_ssql(k);                        // xssql (RXA.c:594)
    tick(2);
    // xwcpagc mode 0 + xpanel, narrowed in the store when the audio frames are fused -- unless every channel's last stage has written
    // the caller's buffer
    if (!k.direct && !k.agc_direct) {
        auto *pass = k.eg_fused ? &pointwise_kernel<double, false, true> : &pointwise_kernel<double, false>;
        const EgressFmt pass_eg = k.eg_fused ? eg : EgressFmt{};
        if (lists[L_PLAIN].n) hipLaunchKernelGGL(pass, dim3(gx, (unsigned)lists[L_PLAIN].n), dim3(NT), 0, stream, k.cur, buf_cap, k.out, k.out_stride, (int)n_mid,
                                        (const unsigned long long *)nullptr, (const unsigned long long *)nullptr, epi, lists[L_PLAIN].dev, pass_eg);
        if (lists[L_BP1].n) hipLaunchKernelGGL(pass, dim3(gx, (unsigned)lists[L_BP1].n), dim3(NT), 0, stream, k.other, buf_cap, k.out, k.out_stride, (int)n_mid,
                                      (const unsigned long long *)nullptr, (const unsigned long long *)nullptr, epi, lists[L_BP1].dev, pass_eg);
    }
    if (lists[L_AMSQ].n) hipLaunchKernelGGL(amsq_apply_kernel, dim3((unsigned)lists[L_AMSQ].n), dim3(64), 0, stream, k.out, k.out_stride, (int)n_mid, lists[L_AMSQ].dev,
                                   amsq_mag, amsq_mag_cap, amsq_prm, amsq_state, amsq_cup, amsq_cdown);       // xamsq, RXA.c:596
    if (eg.kind && !k.eg_fused) pack_audio(k.out, k.out_stride, n_mid);
    tick(3);
}

}  // namespace qh

// ------------------------------------------------------------------------------------------ C ABI
using namespace qh;

// One lock per engine: setters may come from another thread than the one that runs the blocks (Quisk's GUI thread against its
// sound thread; WDSP's setters take csDSP).  A setter only edits the host-side configuration and marks it dirty; the next
// process call uploads what changed before it enqueues the block, so parameters swap on a block boundary.
struct qh_rxa { Engine e; std::recursive_mutex mtx; };
#define QH_RXA_LOCK(h) std::lock_guard<std::recursive_mutex> _lk((h)->mtx)

extern "C" {

int qh_version(void) { return 100; }
const char *qh_last_error(void) { return g_last_error.c_str(); }

int qh_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

qh_rxa *qh_rxa_create(int device, int nch, int dsp_size, int in_rate, int dsp_rate, int out_rate, void *stream)
{
    if (nch <= 0 || dsp_size <= 0 || (dsp_size & (dsp_size - 1)) || in_rate <= 0 || dsp_rate <= 0) {
        set_error(QH_ERR_INVALID, "qh_rxa_create: bad arguments");
        return nullptr;
    }
    if (out_rate <= 0 || (out_rate % dsp_rate && dsp_rate % out_rate) || (out_rate < dsp_rate && dsp_size % (dsp_rate / out_rate))) {
        set_error(QH_ERR_UNSUPPORTED, "out_rate must be an integer multiple or fraction of dsp_rate (wdsp/channel.c:47-52)");
        return nullptr;
    }
    // in_rate / dsp_rate 1, 2, 4, 8, 16: the overlap-save front stage.  Any other whole ratio, up or down (3, 5, 6 ...; 1/2,
    // 1/4 ...): xshift as a pointwise pass + the polyphase form of xresample (wdsp/resample.c:35-157) -- D = 0 marks it.  The
    // reference sizes its blocks with integer divisions of the two rates (pre_main_build, wdsp/channel.c:39-42): a ratio that is
    // not whole one way or the other does not give it consistent block sizes, and is refused here.
    int D = (in_rate % dsp_rate) ? 0 : in_rate / dsp_rate;
    if (D != 1 && D != 2 && D != 4 && D != 8 && D != 16) D = 0;
    if (D == 0 && !((in_rate > dsp_rate && in_rate % dsp_rate == 0) ||
                    (in_rate < dsp_rate && dsp_rate % in_rate == 0 && dsp_size % (dsp_rate / in_rate) == 0))) {
        // (a CPU test of the reference's arithmetic, test_rates_that_are_whole_in_neither_direction_recycle_stale_buffer_tails, shows what it
        // does with 96 k -> 64 k -> 48 k: every block's tail is what the block before left in the buffer)
        set_error(QH_ERR_UNSUPPORTED, "in_rate / dsp_rate must be a whole number or the reciprocal of one (wdsp/channel.c:39-42)");
        return nullptr;
    }
    if (qh_device_count() <= device || device < 0) {
        set_error(QH_ERR_NO_DEVICE, "no HIP device %d (libquiskhip has no CPU fallback)", device);
        return nullptr;
    }
    qh_rxa *h = new qh_rxa();
    h->e.device = device; h->e.nch = nch; h->e.dsp_size = dsp_size;
    h->e.in_rate = in_rate; h->e.dsp_rate = dsp_rate; h->e.out_rate = out_rate; h->e.D = D;
    h->e.stream = (hipStream_t)stream;
    if (h->e.init() != QH_OK) { delete h; return nullptr; }
    return h;
}

void qh_rxa_destroy(qh_rxa *h) { delete h; }
int qh_rxa_nch(const qh_rxa *h) { return h->e.nch; }
int qh_rxa_dsp_insize(const qh_rxa *h) { return h->e.dsp_insize; }
int qh_rxa_dsp_outsize(const qh_rxa *h) { return h->e.dsp_outsize; }
void *qh_rxa_stream(const qh_rxa *h) { return h ? (void *)h->e.stream : nullptr; }
long long qh_rxa_device_bytes(const qh_rxa *h) { return h->e.dev_bytes(); }

#define FOR_CH(h, ch, body)                                                                       \
    do {                                                                                          \
        if (!(h)) return set_error(QH_ERR_INVALID, "null engine");                                \
        QH_RXA_LOCK(h);                                                                           \
        if ((ch) < -1 || (ch) >= (h)->e.nch) return set_error(QH_ERR_INVALID, "channel %d out of range", (ch)); \
        int _lo = (ch) < 0 ? 0 : (ch), _hi = (ch) < 0 ? (h)->e.nch : (ch) + 1;                    \
        (h)->e.epoch++;                                                                           \
        for (int _i = _lo; _i < _hi; _i++) { ChanCfg &c = (h)->e.cfg[(size_t)_i]; body }         \
        return QH_OK;                                                                             \
    } while (0)

// RXAbp1Check + RXAbp1Set, wdsp/RXA.c:800-827 (snba/emnr/anf/anr never run here)
static void bp1_check_set(ChanCfg &c, int amd_run, int anf_run, int anr_run, int emnr_run = -1, int snba_run = -1)
{
    if (emnr_run < 0) emnr_run = c.emnr_run;
    if (snba_run < 0) snba_run = c.snba_run;
    const double gain = (amd_run || anf_run || anr_run || emnr_run || snba_run) ? 2.0 : 1.0;
    if (c.bp1_gain != gain) { c.bp1_gain = gain; c.bp1_dirty = true; }
}
static void bp1_set(ChanCfg &c)
{
    const int old = c.bp1_run;
    c.bp1_run = (c.amd_run || c.lms[0].run || c.lms[1].run || c.emnr_run || c.snba_run) ? 1 : 0;
    if (old != c.bp1_run) c.bp1_dirty = true;
    if (!old && c.bp1_run) c.bp1_flush = true;
}

int qh_rxa_SetRXAMode(qh_rxa *h, int ch, int mode)
{
    FOR_CH(h, ch, {
        if (c.mode != mode) {       // wdsp/RXA.c:748-787
            const int amd_run = (mode == QH_AM) || (mode == QH_SAM);
            bp1_check_set(c, amd_run, c.lms[0].run, c.lms[1].run);
            c.mode = mode;
            c.amd_run = 0; c.fmd_run = 0; c.agc_run = 1;
            if (mode == QH_AM) { c.amd_run = 1; c.amd_mode = 0; }
            else if (mode == QH_SAM) { c.amd_run = 1; c.amd_mode = 1; }
            else if (mode == QH_FM) { c.fmd_run = 1; c.agc_run = 0; }
            bp1_set(c);
            c.snb_dirty = true;
            c.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}

// SetRXAAMDRun (wdsp/amd.c:264-277): the AM demodulator's run flag on its own (SetRXAMode sets it from the mode)
int qh_rxa_SetRXAAMDRun(qh_rxa *h, int ch, int run)
{
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.amd_run != run) {
            bp1_check_set(c, run, c.lms[0].run, c.lms[1].run);
            c.amd_run = run;
            bp1_set(c);
            c.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}

int qh_rxa_SetRXABandpassFreqs(qh_rxa *h, int ch, double f_low, double f_high)
{
    FOR_CH(h, ch, {
        if (f_low != c.bp1_flow || f_high != c.bp1_fhigh) { c.bp1_flow = f_low; c.bp1_fhigh = f_high; c.bp1_dirty = true; }
    });
}

int qh_rxa_RXANBPSetFreqs(qh_rxa *h, int ch, double flow, double fhigh)
{
    FOR_CH(h, ch, {
        if (flow != c.nbp_flow || fhigh != c.nbp_fhigh) { c.nbp_flow = flow; c.nbp_fhigh = fhigh; c.nbp_dirty = true; }
    });
}

// SetRXASNBAOutputBandwidth, wdsp/snb.c:660-694: the pass band of the blanker's 12 kHz -> dsp_rate resampler
int qh_rxa_SetRXASNBAOutputBandwidth(qh_rxa *h, int ch, double flow, double fhigh)
{
    FOR_CH(h, ch, {
        const double lc = 200.0;        // out_low_cut / out_high_cut, RXA.c:254-255
        const double hc = 5400.0;
        double lo = flow;
        double hi = fhigh;
        double f_low = c.snba_f_low;
        double f_high = c.snba_f_high;
        if (lo >= 0 && hi >= 0) {
            if (hi < lc) hi = lc;
            if (lo > hc) lo = hc;
            f_low = lc > lo ? lc : lo;
            f_high = hc < hi ? hc : hi;
        } else if (lo <= 0 && hi <= 0) {
            if (lo > -lc) lo = -lc;
            if (hi < -hc) hi = -hc;
            f_low = lc > -hi ? lc : -hi;
            f_high = hc < -lo ? hc : -lo;
        } else if (lo < 0 && hi > 0) {
            double absmax = -lo > hi ? -lo : hi;
            if (absmax < lc) absmax = lc;
            f_low = lc;
            f_high = hc < absmax ? hc : absmax;
        }
        if (f_low != c.snba_f_low || f_high != c.snba_f_high) {     // setBandwidth_resample rebuilds the filter and clears its ring
            c.snba_f_low = f_low; c.snba_f_high = f_high;
            c.snba_taps_dirty = true; c.snba_rout_flush = true;
            c.epi_dirty = true;
        }
    });
}

// The blanker's tuning setters, wdsp/snb.c:604-658.  They act on the next block, as under csDSP.
static int snba_tune_set(qh_rxa *h, int ch, const char *who, bool ok, void (*apply)(SnbaTune &, double), double v)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    if (!ok) return set_error(QH_ERR_INVALID, "%s: value out of range", who);
    QH_RXA_LOCK(h);
    if (ch < -1 || ch >= h->e.nch) return set_error(QH_ERR_INVALID, "channel out of range");
    for (int c = ch < 0 ? 0 : ch; c < (ch < 0 ? h->e.nch : ch + 1); c++) apply(h->e.snba_tune_h[(size_t)c], v);
    h->e.snba_tune_dirty = true;
    h->e.drop_graphs(); h->e.epoch++;
    return QH_OK;
}
int qh_rxa_SetRXASNBAasize(qh_rxa *h, int ch, int size)
{ return snba_tune_set(h, ch, "SetRXASNBAasize (1 .. 64)", size >= 1 && size <= 64, [](SnbaTune &t, double v) { t.asize = (int)v; }, size); }
int qh_rxa_SetRXASNBAnpasses(qh_rxa *h, int ch, int npasses)
{ return snba_tune_set(h, ch, "SetRXASNBAnpasses (0 .. 8)", npasses >= 0 && npasses <= 8, [](SnbaTune &t, double v) { t.npasses = (int)v; }, npasses); }
int qh_rxa_SetRXASNBAk1(qh_rxa *h, int ch, double k1)
{ return snba_tune_set(h, ch, "SetRXASNBAk1", k1 > 0.0, [](SnbaTune &t, double v) { t.k1 = v; }, k1); }
int qh_rxa_SetRXASNBAk2(qh_rxa *h, int ch, double k2)
{ return snba_tune_set(h, ch, "SetRXASNBAk2", k2 > 0.0, [](SnbaTune &t, double v) { t.k2 = v; }, k2); }
int qh_rxa_SetRXASNBAbridge(qh_rxa *h, int ch, int bridge)
{ return snba_tune_set(h, ch, "SetRXASNBAbridge (0 .. 64)", bridge >= 0 && bridge <= 64, [](SnbaTune &t, double v) { t.b = (int)v; }, bridge); }
int qh_rxa_SetRXASNBApresamps(qh_rxa *h, int ch, int presamps)
{ return snba_tune_set(h, ch, "SetRXASNBApresamps (0 .. 64)", presamps >= 0 && presamps <= 64, [](SnbaTune &t, double v) { t.pre = (int)v; }, presamps); }
int qh_rxa_SetRXASNBApostsamps(qh_rxa *h, int ch, int postsamps)
{ return snba_tune_set(h, ch, "SetRXASNBApostsamps (0 .. 64)", postsamps >= 0 && postsamps <= 64, [](SnbaTune &t, double v) { t.post = (int)v; }, postsamps); }
int qh_rxa_SetRXASNBApmultmin(qh_rxa *h, int ch, double pmultmin)
{ return snba_tune_set(h, ch, "SetRXASNBApmultmin", pmultmin >= 0.0, [](SnbaTune &t, double v) { t.pmultmin = v; }, pmultmin); }

// SetRXASNBAovrlp, wdsp/snb.c:595-603.  The frame advance sizes the blanker's state, which the engine lays out once for all its
// channels: ch = -1 (or the only channel).  The WDSP-named layer keeps one engine per channel, so there it is per channel as in WDSP.
int qh_rxa_SetRXASNBAovrlp(qh_rxa *h, int ch, int ovrlp)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (!(ch == -1 || (ch == 0 && h->e.nch == 1)))
        return set_error(QH_ERR_UNSUPPORTED, "SetRXASNBAovrlp re-plans the blanker's accumulators for the whole engine: pass channel -1");
    if (int rc = h->e.snba_set_ovrlp(ovrlp)) return rc;
    // calc_snba makes the output resampler anew with its creation arguments: fc_low 200, the default cut-off (snb.c:45-46) -- what
    // SetRXASNBAOutputBandwidth had set is gone, as in WDSP
    for (ChanCfg &c : h->e.cfg) { c.snba_f_low = 200.0; c.snba_f_high = 0.0; c.snba_taps_dirty = true; }
    return QH_OK;
}

// SetRXASNBARun, wdsp/snb.c:579-593
int qh_rxa_SetRXASNBARun(qh_rxa *h, int ch, int run)
{
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.snba_run != run) {
            bp1_check_set(c, c.amd_run, c.lms[0].run, c.lms[1].run, -1, run);
            c.snba_run = run;
            bp1_set(c);
            c.snb_dirty = true;
            c.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}

int qh_rxa_RXASetPassband(qh_rxa *h, int ch, double f_low, double f_high)
{
    int rc = qh_rxa_SetRXABandpassFreqs(h, ch, f_low, f_high);
    if (rc) return rc;
    if ((rc = qh_rxa_SetRXASNBAOutputBandwidth(h, ch, f_low, f_high))) return rc;
    return qh_rxa_RXANBPSetFreqs(h, ch, f_low, f_high);
}

int qh_rxa_RXASetNC(qh_rxa *h, int ch, int nc)
{
    if (nc < 1 || (nc & (nc - 1)) || nc > kLongNcMax || (h && nc < h->e.dsp_size))
        return set_error(QH_ERR_UNSUPPORTED, "nc must be a power of two in [dsp_size, %d]", kLongNcMax);
    FOR_CH(h, ch, {
        if (c.nbp_nc != nc) { c.nbp_nc = nc; c.nbp_dirty = true; c.nbp_flush = true; c.snb_flush = true; c.long_live[0] = c.long_live[4] = false; }
        if (c.bp1_nc != nc) { c.bp1_nc = nc; c.bp1_dirty = true; c.bp1_flush = true; c.long_live[1] = false; }
        if (c.fm_nc != nc) c.long_live[2] = false;     // (setNc_fircore zeroes the delay lines, firmin.c:454-466: nothing long is held any more)
        c.fm_nc = nc;                           // SetRXAFMNCde / SetRXAFMNCaud, wdsp/RXA.c:942-943
    });
}

static Notch mk_notch(double fcenter, double fwidth, int active)
{
    Notch n;
    n.fcenter = fcenter; n.fwidth = fwidth; n.active = active;
    return n;
}

// ---- the notch database (wdsp/nbp.c:358-525).  Return values of Add / Delete / Edit / Get follow the reference:
// 0, or -1 for an index out of range (reported through *rval; the function result stays the library's status).
int qh_rxa_RXANBPAddNotch(qh_rxa *h, int ch, int notch, double fcenter, double fwidth, int active, int *rval)
{
    if (rval) *rval = -1;
    FOR_CH(h, ch, {
        if (notch >= 0 && notch <= (int)c.notches.size() && c.notches.size() < 1024) {
            c.notches.insert(c.notches.begin() + notch, mk_notch(fcenter, fwidth, active));
            if (c.fnfrun) c.nbp_dirty = true;
            if (rval) *rval = 0;
        } else if (rval) *rval = -1;
    });
}

int qh_rxa_RXANBPDeleteNotch(qh_rxa *h, int ch, int notch, int *rval)
{
    if (rval) *rval = -1;
    FOR_CH(h, ch, {
        if (notch >= 0 && notch < (int)c.notches.size()) {
            c.notches.erase(c.notches.begin() + notch);
            if (c.fnfrun) c.nbp_dirty = true;
            if (rval) *rval = 0;
        } else if (rval) *rval = -1;
    });
}

int qh_rxa_RXANBPEditNotch(qh_rxa *h, int ch, int notch, double fcenter, double fwidth, int active, int *rval)
{
    if (rval) *rval = -1;
    FOR_CH(h, ch, {
        if (notch >= 0 && notch < (int)c.notches.size()) {
            c.notches[(size_t)notch] = mk_notch(fcenter, fwidth, active);
            if (c.fnfrun) c.nbp_dirty = true;
            if (rval) *rval = 0;
        } else if (rval) *rval = -1;
    });
}

int qh_rxa_RXANBPGetNotch(qh_rxa *h, int ch, int notch, double *fcenter, double *fwidth, int *active, int *rval)
{
    if (!h || ch < 0 || ch >= h->e.nch || !fcenter || !fwidth || !active) return set_error(QH_ERR_INVALID, "RXANBPGetNotch: bad arguments");
    const ChanCfg &c = h->e.cfg[(size_t)ch];
    if (notch >= 0 && notch < (int)c.notches.size()) {
        *fcenter = c.notches[(size_t)notch].fcenter; *fwidth = c.notches[(size_t)notch].fwidth; *active = c.notches[(size_t)notch].active;
        if (rval) *rval = 0;
    } else {
        *fcenter = -1.0; *fwidth = 0.0; *active = -1;
        if (rval) *rval = -1;
    }
    return QH_OK;
}

int qh_rxa_RXANBPGetNumNotches(qh_rxa *h, int ch, int *nnotches)
{
    if (!h || ch < 0 || ch >= h->e.nch || !nnotches) return set_error(QH_ERR_INVALID, "RXANBPGetNumNotches: bad arguments");
    *nnotches = (int)h->e.cfg[(size_t)ch].notches.size();
    return QH_OK;
}

int qh_rxa_RXANBPGetMinNotchWidth(qh_rxa *h, int ch, double *minwidth)
{
    if (!h || ch < 0 || ch >= h->e.nch || !minwidth) return set_error(QH_ERR_INVALID, "RXANBPGetMinNotchWidth: bad arguments");
    const ChanCfg &c = h->e.cfg[(size_t)ch];
    *minwidth = (c.nbp_wintype == 1 ? 2200.0 : 1600.0) / (c.nbp_nc / 256) * ((double)h->e.dsp_rate / 48000);      // nbp.c:82-95
    return QH_OK;
}

int qh_rxa_RXANBPSetTuneFrequency(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { if (f != c.ndb_tunefreq) { c.ndb_tunefreq = f; if (c.fnfrun) c.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetShiftFrequency(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { if (f != c.ndb_shift) { c.ndb_shift = f; if (c.fnfrun) c.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetNotchesRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { run = run ? 1 : 0; if (run != c.fnfrun) { c.fnfrun = run; c.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetWindow(qh_rxa *h, int ch, int wintype) { FOR_CH(h, ch, { if (c.nbp_wintype != wintype) { c.nbp_wintype = wintype; c.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetAutoIncrease(qh_rxa *h, int ch, int autoincr) { FOR_CH(h, ch, { if (c.autoincr != autoincr) { c.autoincr = autoincr; if (c.fnfrun) c.nbp_dirty = true; } }); }

// RXASetMP (wdsp/RXA.c:948-958): minimum-phase impulse responses in every fircore of the chain.  nbp0 and bp1 have
// per-channel masks; the FM de-emphasis / audio masks are shared by the channels of an engine and follow the
// most recent call.
int qh_rxa_RXASetMP(qh_rxa *h, int ch, int mp)
{
    mp = mp ? 1 : 0;
    FOR_CH(h, ch, {
        if (c.mp != mp) { c.mp = mp; c.nbp_dirty = true; c.bp1_dirty = true; c.demod_dirty = true; }
    });
}

int qh_rxa_SetRXAShiftRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.shift_run = run; c.nco_dirty = true; }); }
int qh_rxa_SetRXAShiftFreq(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { c.shift_freq = f; c.nco_dirty = true; }); }
int qh_rxa_RXANBPSetRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { if (c.nbp_run != run) { c.nbp_run = run; c.nbp_dirty = true; } }); }
// (bandpass.c:385-390 writes the flag and nothing else; where a fixed AGC gain is applied -- at the AGC's own spot or in the output matrix --
// depends on it: fix_before)
int qh_rxa_SetRXABandpassRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { if (c.bp1_run != run) { c.bp1_run = run; c.bp1_dirty = true; c.epi_dirty = true; h->e.lists_dirty = true; } }); }
int qh_rxa_SetRXAAMDSBMode(qh_rxa *h, int ch, int sbmode) { FOR_CH(h, ch, { c.sbmode = sbmode; c.demod_dirty = true; }); }
int qh_rxa_SetRXAAMDFadeLevel(qh_rxa *h, int ch, int levelfade) { FOR_CH(h, ch, { c.levelfade = levelfade; c.demod_dirty = true; }); }
int qh_rxa_SetRXAFMDeviation(qh_rxa *h, int ch, double deviation) { FOR_CH(h, ch, { c.fm_dev = deviation; c.demod_dirty = true; }); }
int qh_rxa_SetRXACTCSSFreq(qh_rxa *h, int ch, double freq) { FOR_CH(h, ch, { c.ctcss_freq = freq; c.demod_dirty = true; c.ctcss_flush = true; }); }
int qh_rxa_SetRXACTCSSRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.ctcss_run = run; c.demod_dirty = true; }); }
// SetRXAFMLimRun / SetRXAFMLimGain (wdsp/fmd.c:336-362): the FM detector's limiter
int qh_rxa_SetRXAFMLimRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { run = run ? 1 : 0; if (c.lim_run != run) { c.lim_run = run; h->e.lists_dirty = true; } }); }
int qh_rxa_SetRXAFMLimGain(qh_rxa *h, int ch, double gaindB)
{
    const double gain = std::pow(10.0, gaindB / 20.0);
    FOR_CH(h, ch, { if (c.lim_gain != gain) { c.lim_gain = gain; c.lim_dirty = true; } });
}

// SetRXAEMNRRun ... SetRXAEMNRPosition, wdsp/emnr.c:1096-1143
int qh_rxa_SetRXAEMNRRun(qh_rxa *h, int ch, int run)
{
    if (h && run && !h->e.emnr_tables)
        return set_error(QH_ERR_INVALID, "EMNR needs its gain tables first (qh_rxa_SetEMNRTables: WDSP's `calculus` and `zetaHat.bin` data)");
    if (h && run && h->e.dsp_size > kEmnrIncr) return set_error(QH_ERR_UNSUPPORTED, "EMNR: dsp_size up to %d", kEmnrIncr);
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.emnr_run != run) {
            bp1_check_set(c, c.amd_run, c.lms[0].run, c.lms[1].run, run);
            c.emnr_run = run;
            bp1_set(c);
            c.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}
int qh_rxa_SetRXAEMNRgainMethod(qh_rxa *h, int ch, int method) { FOR_CH(h, ch, { c.emnr_gain_method = method; c.emnr_dirty = true; }); }
int qh_rxa_SetRXAEMNRnpeMethod(qh_rxa *h, int ch, int method) { FOR_CH(h, ch, { c.emnr_npe = method; c.emnr_dirty = true; }); }
int qh_rxa_SetRXAEMNRaeRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.emnr_ae = run ? 1 : 0; c.emnr_dirty = true; }); }
int qh_rxa_SetRXAEMNRaeZetaThresh(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_ae_zeta = v; c.emnr_dirty = true; }); }       // emnr.c:1145
int qh_rxa_SetRXAEMNRaePsi(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_ae_psi = v; c.emnr_dirty = true; }); }               // emnr.c:1153
int qh_rxa_SetRXAEMNRtrainZetaThresh(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_train_zeta = v; c.emnr_dirty = true; }); }  // emnr.c:1161
int qh_rxa_SetRXAEMNRtrainT2(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_train_t2 = v; c.emnr_dirty = true; }); }            // emnr.c:1169
int qh_rxa_SetRXAEMNRPosition(qh_rxa *h, int ch, int position)
{
    FOR_CH(h, ch, { c.emnr_pos = position ? 1 : 0; c.bp1_pos = position ? 1 : 0; c.epi_dirty = true; h->e.lists_dirty = true; });
}
// The data WDSP reads at create time from the files `calculus` (GG, GGS: 241 x 241 each) and `zetaHat.bin` (60 x 60 values, validity
// flags and their gamma / xi ranges in dB), emnr.c:206-238,317-334
int qh_rxa_SetEMNRTables(qh_rxa *h, const double *GG, const double *GGS, const double *zeta_hat, const int *zeta_true, double gamma_min,
                         double gamma_max, double xi_min, double xi_max)
{
    if (!h || !GG || !GGS || !zeta_hat || !zeta_true) return set_error(QH_ERR_INVALID, "qh_rxa_SetEMNRTables: null table");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    e.epoch++;
    e.h_GG.assign(GG, GG + 241 * 241); e.h_GGS.assign(GGS, GGS + 241 * 241);
    e.h_zeta.assign(zeta_hat, zeta_hat + 3600); e.h_zeta_true.assign(zeta_true, zeta_true + 3600);
    e.h_zrange[0] = gamma_min; e.h_zrange[1] = gamma_max; e.h_zrange[2] = xi_min; e.h_zrange[3] = xi_max;
    e.emnr_tables = true;
    if (e.emnr_GG) {            // already on the device: refresh
        QH_HIP(hipSetDevice(e.device));
        QH_HIP(hipMemcpyAsync(e.emnr_GG, GG, 241 * 241 * 8, hipMemcpyHostToDevice, e.stream));
        QH_HIP(hipMemcpyAsync(e.emnr_GGS, GGS, 241 * 241 * 8, hipMemcpyHostToDevice, e.stream));
        QH_HIP(hipMemcpyAsync(e.emnr_zeta, zeta_hat, 3600 * 8, hipMemcpyHostToDevice, e.stream));
        QH_HIP(hipMemcpyAsync(e.emnr_zeta_true, zeta_true, 3600 * 4, hipMemcpyHostToDevice, e.stream));
        QH_HIP(hipStreamSynchronize(e.stream));
        e.emnr_prm.z_gamma_min = gamma_min; e.emnr_prm.z_gamma_max = gamma_max; e.emnr_prm.z_xihat_min = xi_min; e.emnr_prm.z_xihat_max = xi_max;
    }
    return QH_OK;
}

// SetRXAANFRun ... SetRXAANFPosition (wdsp/anf.c:175-239) and the ANR twins (wdsp/anr.c:175-238); which = 0 anf, 1 anr
static int lms_run(qh_rxa *h, int ch, int which, int run)
{
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        ChanCfg::Lms &m = c.lms[which];
        if (m.run != run) {
            bp1_check_set(c, c.amd_run, which == 0 ? run : c.lms[0].run, which == 1 ? run : c.lms[1].run);
            m.run = run;
            bp1_set(c);
            m.flush = true;
            c.lms[0].dirty = c.lms[1].dirty = true; c.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}
static int lms_vals(qh_rxa *h, int ch, int which, const int *taps, const int *delay, const double *gain, const double *leakage)
{
    FOR_CH(h, ch, {
        ChanCfg::Lms &m = c.lms[which];
        if (taps) m.taps = *taps;
        if (delay) m.delay = *delay;
        if (gain) m.two_mu = *gain;
        if (leakage) m.gamma = *leakage;
        m.flush = true; m.dirty = true;
    });
}
static int lms_position(qh_rxa *h, int ch, int which, int position)
{
    FOR_CH(h, ch, {
        c.lms[which].position = position ? 1 : 0;
        c.bp1_pos = position ? 1 : 0;                 // "rxa[channel].bp1.p->position = position", anf.c:236
        c.lms[which].flush = true;
        c.lms[0].dirty = c.lms[1].dirty = true; c.epi_dirty = true;
        h->e.lists_dirty = true;
    });
}
// SetRXAAMSQRun / Threshold / MaxTail, wdsp/amsq.c:216-243
int qh_rxa_SetRXAAMSQRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.amsq_run = run ? 1 : 0; h->e.lists_dirty = true; }); }
int qh_rxa_SetRXAAMSQThreshold(qh_rxa *h, int ch, double threshold)
{
    FOR_CH(h, ch, { const double t = std::pow(10.0, threshold / 20.0); c.amsq_tail_thresh = 0.9 * t; c.amsq_unmute_thresh = t; c.amsq_dirty = true; });
}
int qh_rxa_SetRXAAMSQMaxTail(qh_rxa *h, int ch, double tail) { FOR_CH(h, ch, { c.amsq_max_tail = tail < 0.0 ? 0.0 : tail; c.amsq_dirty = true; }); }
int qh_rxa_SetRXAANFRun(qh_rxa *h, int ch, int run) { return lms_run(h, ch, 0, run); }
int qh_rxa_SetRXAANRRun(qh_rxa *h, int ch, int run) { return lms_run(h, ch, 1, run); }
int qh_rxa_SetRXAANFVals(qh_rxa *h, int ch, int taps, int delay, double gain, double leakage) { return lms_vals(h, ch, 0, &taps, &delay, &gain, &leakage); }
int qh_rxa_SetRXAANRVals(qh_rxa *h, int ch, int taps, int delay, double gain, double leakage) { return lms_vals(h, ch, 1, &taps, &delay, &gain, &leakage); }
int qh_rxa_SetRXAANFTaps(qh_rxa *h, int ch, int taps) { return lms_vals(h, ch, 0, &taps, nullptr, nullptr, nullptr); }
int qh_rxa_SetRXAANRTaps(qh_rxa *h, int ch, int taps) { return lms_vals(h, ch, 1, &taps, nullptr, nullptr, nullptr); }
int qh_rxa_SetRXAANFDelay(qh_rxa *h, int ch, int delay) { return lms_vals(h, ch, 0, nullptr, &delay, nullptr, nullptr); }
int qh_rxa_SetRXAANRDelay(qh_rxa *h, int ch, int delay) { return lms_vals(h, ch, 1, nullptr, &delay, nullptr, nullptr); }
int qh_rxa_SetRXAANFGain(qh_rxa *h, int ch, double gain) { return lms_vals(h, ch, 0, nullptr, nullptr, &gain, nullptr); }
int qh_rxa_SetRXAANRGain(qh_rxa *h, int ch, double gain) { return lms_vals(h, ch, 1, nullptr, nullptr, &gain, nullptr); }
int qh_rxa_SetRXAANFLeakage(qh_rxa *h, int ch, double leakage) { return lms_vals(h, ch, 0, nullptr, nullptr, nullptr, &leakage); }
int qh_rxa_SetRXAANRLeakage(qh_rxa *h, int ch, double leakage) { return lms_vals(h, ch, 1, nullptr, nullptr, nullptr, &leakage); }
int qh_rxa_SetRXAANFPosition(qh_rxa *h, int ch, int position) { return lms_position(h, ch, 0, position); }
int qh_rxa_SetRXAANRPosition(qh_rxa *h, int ch, int position) { return lms_position(h, ch, 1, position); }

int qh_rxa_SetRXAAGCMode(qh_rxa *h, int ch, int mode)
{
    FOR_CH(h, ch, {                 // wdsp/wcpAGC.c:369-411
        switch (mode) {
        case 0: c.agc_mode = 0; break;
        case 1: c.agc_mode = 1; c.agc_hangtime = 2.000; c.agc_tau_decay = 2.000; break;
        case 2: c.agc_mode = 2; c.agc_hangtime = 1.000; c.agc_tau_decay = 0.500; break;
        case 3: c.agc_mode = 3; c.agc_hang_thresh = 1.0; c.agc_hangtime = 0.000; c.agc_tau_decay = 0.250; break;
        case 4: c.agc_mode = 4; c.agc_hang_thresh = 1.0; c.agc_hangtime = 0.000; c.agc_tau_decay = 0.050; break;
        default: c.agc_mode = 5; break;
        }
        c.epi_dirty = true; c.agc_dirty = true; c.lms[0].dirty = c.lms[1].dirty = true; h->e.lists_dirty = true;
    });
}
int qh_rxa_SetRXAAGCAttack(qh_rxa *h, int ch, int attack_ms) { FOR_CH(h, ch, { c.agc_tau_attack = (double)attack_ms / 1000.0; c.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCDecay(qh_rxa *h, int ch, int decay_ms) { FOR_CH(h, ch, { c.agc_tau_decay = (double)decay_ms / 1000.0; c.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCHang(qh_rxa *h, int ch, int hang_ms) { FOR_CH(h, ch, { c.agc_hangtime = (double)hang_ms / 1000.0; c.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCTop(qh_rxa *h, int ch, double max_agc_db) { FOR_CH(h, ch, { c.agc_max_gain = std::pow(10.0, max_agc_db / 20.0); c.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCSlope(qh_rxa *h, int ch, int slope) { FOR_CH(h, ch, { c.agc_var_gain = std::pow(10.0, (double)slope / 20.0 / 10.0); c.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCHangThreshold(qh_rxa *h, int ch, int t) { FOR_CH(h, ch, { c.agc_hang_thresh = (double)t / 100.0; c.agc_dirty = true; }); }

int qh_rxa_SetRXAAGCFixed(qh_rxa *h, int ch, double db)
{
    FOR_CH(h, ch, { c.agc_fixed = std::pow(10.0, db / 20.0); c.epi_dirty = true; c.lms[0].dirty = c.lms[1].dirty = true; });
}

// xcbl / xspeak / xmpeak.  Run flags, npeaks and the enables do not flush (cblock.c:120-126, iir.c:322-330, :490-515); the design
// setters recompute and zero their cascade -- speak's, or that one peak's (calc_speak ends in flush_speak, iir.c:216, :332-360, :517-548).
// npeaks outside [0, 2] and fil outside [0, 2) would index past the reference's two-peak arrays: refused, nothing changes.
static void ap_run_set(qh_rxa *h, ChanCfg &c, int &flag, int run)
{
    run = run ? 1 : 0;
    if (flag == run) return;
    flag = run;
    c.ap_dirty = true; c.epi_dirty = true;          // fix_before() follows ap_on()
    h->e.lists_dirty = true;
}
int qh_rxa_SetRXACBLRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { ap_run_set(h, c, c.cbl_run, run); }); }
int qh_rxa_SetRXASPCWRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { ap_run_set(h, c, c.sp_run, run); }); }
int qh_rxa_SetRXASPCWFreq(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { c.sp_f = f < 200.0 ? 200.0 : f; c.ap_dirty = true; c.sp_flush = true; }); }
int qh_rxa_SetRXASPCWBandwidth(qh_rxa *h, int ch, double bw) { FOR_CH(h, ch, { c.sp_bw = bw; c.ap_dirty = true; c.sp_flush = true; }); }
int qh_rxa_SetRXASPCWGain(qh_rxa *h, int ch, double g) { FOR_CH(h, ch, { c.sp_gain = g; c.ap_dirty = true; c.sp_flush = true; }); }
int qh_rxa_SetRXAmpeakRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { ap_run_set(h, c, c.mp_run, run); }); }
int qh_rxa_SetRXAmpeakNpeaks(qh_rxa *h, int ch, int npeaks)
{
    if (npeaks < 0 || npeaks > kApPeaks) return set_error(QH_ERR_INVALID, "SetRXAmpeakNpeaks: npeaks %d outside [0, %d]", npeaks, kApPeaks);
    FOR_CH(h, ch, { if (c.mp_npeaks != npeaks) { c.mp_npeaks = npeaks; c.ap_dirty = true; } });
}
int qh_rxa_SetRXAmpeakFilEnable(qh_rxa *h, int ch, int fil, int enable)
{
    if (fil < 0 || fil >= kApPeaks) return set_error(QH_ERR_INVALID, "SetRXAmpeakFilEnable: fil %d outside [0, %d)", fil, kApPeaks);
    FOR_CH(h, ch, { enable = enable ? 1 : 0; if (c.mp_enable[fil] != enable) { c.mp_enable[fil] = enable; c.ap_dirty = true; } });
}
static int mpeak_design(qh_rxa *h, int ch, int fil, int what, double v)
{
    if (fil < 0 || fil >= kApPeaks) return set_error(QH_ERR_INVALID, "SetRXAmpeakFil*: fil %d outside [0, %d)", fil, kApPeaks);
    FOR_CH(h, ch, {
        if (what == 0) c.mp_f[fil] = v < 200.0 ? 200.0 : v;
        else if (what == 1) c.mp_bw[fil] = v;
        else c.mp_gain[fil] = v;
        c.ap_dirty = true; c.mp_flush[fil] = true;
    });
}
int qh_rxa_SetRXAmpeakFilFreq(qh_rxa *h, int ch, int fil, double f) { return mpeak_design(h, ch, fil, 0, f); }
int qh_rxa_SetRXAmpeakFilBw(qh_rxa *h, int ch, int fil, double bw) { return mpeak_design(h, ch, fil, 1, bw); }
int qh_rxa_SetRXAmpeakFilGain(qh_rxa *h, int ch, int fil, double g) { return mpeak_design(h, ch, fil, 2, g); }

// xssql (ssql.c:330-370).  No setter flushes; SetRXASSQLThreshold keeps half its argument; each tau setter recomputes its own
// multiplier.  A tau below 0 or not finite, and a threshold that is not finite, are refused and change nothing (the reference's
// trigger recurrence diverges on them); a tau of 0 gives a multiplier of 1, as there.
int qh_rxa_SetRXASSQLRun(qh_rxa *h, int ch, int run)
{
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.ssql_run != run) { c.ssql_run = run; c.ssql_dirty = true; c.epi_dirty = true; h->e.lists_dirty = true; }   // fix_before() follows
    });
}
int qh_rxa_SetRXASSQLThreshold(qh_rxa *h, int ch, double threshold)
{
    if (!std::isfinite(threshold)) return set_error(QH_ERR_INVALID, "SetRXASSQLThreshold: threshold %g is not finite", threshold);
    FOR_CH(h, ch, { c.ssql_wthresh = threshold / 2.0; c.ssql_dirty = true; });
}
int qh_rxa_SetRXASSQLTauMute(qh_rxa *h, int ch, double tau)
{
    if (!std::isfinite(tau) || tau < 0.0) return set_error(QH_ERR_INVALID, "SetRXASSQLTauMute: tau %g is negative or not finite", tau);
    FOR_CH(h, ch, { c.ssql_tau_mute = tau; c.ssql_dirty = true; });
}
int qh_rxa_SetRXASSQLTauUnMute(qh_rxa *h, int ch, double tau)
{
    if (!std::isfinite(tau) || tau < 0.0) return set_error(QH_ERR_INVALID, "SetRXASSQLTauUnMute: tau %g is negative or not finite", tau);
    FOR_CH(h, ch, { c.ssql_tau_unmute = tau; c.ssql_dirty = true; });
}

int qh_rxa_SetRXAPanelGain1(qh_rxa *h, int ch, double g) { FOR_CH(h, ch, { c.gain1 = g; c.epi_dirty = true; }); }
int qh_rxa_SetRXAPanelGain2(qh_rxa *h, int ch, double gI, double gQ) { FOR_CH(h, ch, { c.gain2I = gI; c.gain2Q = gQ; c.epi_dirty = true; }); }
int qh_rxa_SetRXAPanelSelect(qh_rxa *h, int ch, int s) { FOR_CH(h, ch, { c.inselect = s; c.epi_dirty = true; }); }
int qh_rxa_SetRXAPanelCopy(qh_rxa *h, int ch, int cp) { FOR_CH(h, ch, { c.copy = cp; c.epi_dirty = true; }); }

int qh_rxa_process(qh_rxa *h, const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (!d_in || !d_out) return set_error(QH_ERR_INVALID, "null buffer");
    if (in_stride < (long long)nblk * h->e.dsp_insize || out_stride < (long long)nblk * h->e.dsp_outsize)
        return set_error(QH_ERR_INVALID, "stride shorter than nblk blocks");
    if (h->e.graph_on) return h->e.process_replayed(d_in, in_stride, d_out, out_stride, nblk);
    return h->e.process(d_in, in_stride, d_out, out_stride, nblk);
}

// ---- audio egress ---------------------------------------------------------------------------------------------------
static long long egress_frame_bytes(const qh_audio_format *fmt)        // (a format make_egress has accepted)
{
    return (long long)fmt->num_channels * (fmt->kind == QH_AUDIO_I16 ? 2 : fmt->kind == QH_AUDIO_I24 ? 3 : 4);
}

static int make_egress(const qh_audio_format *fmt, void *d_out, long long out_stride_bytes, long long frames, EgressFmt *f)
{
    if (!fmt || !d_out) return set_error(QH_ERR_INVALID, "null audio format or buffer");
    if (fmt->kind < QH_AUDIO_I16 || fmt->kind > QH_AUDIO_F32) return set_error(QH_ERR_INVALID, "audio kind %d", fmt->kind);
    if (fmt->num_channels < 1 || fmt->channel_I < 0 || fmt->channel_Q < 0 || fmt->channel_I >= fmt->num_channels ||
        fmt->channel_Q >= fmt->num_channels)
        return set_error(QH_ERR_INVALID, "audio channel slots outside the frame");
    const int bytes = egress_frame_bytes(fmt) / fmt->num_channels;
    if (out_stride_bytes < frames * fmt->num_channels * bytes) return set_error(QH_ERR_INVALID, "audio row stride shorter than the frames");
    if (fmt->kind != QH_AUDIO_I24 && out_stride_bytes % bytes) return set_error(QH_ERR_INVALID, "audio row stride not a multiple of the sample size");
    f->kind = fmt->kind; f->nchan = fmt->num_channels; f->ch_i = fmt->channel_I; f->ch_q = fmt->channel_Q;
    f->volume = fmt->volume; f->prescale = fmt->prescale == 0.0 ? 1.0 : fmt->prescale;
    f->out = static_cast<unsigned char *>(d_out); f->stride = out_stride_bytes;
    return QH_OK;
}

int qh_rxa_process_audio(qh_rxa *h, const double *d_in, long long in_stride, void *d_out, long long out_stride_bytes, int nblk,
                         const qh_audio_format *fmt)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (!d_in) return set_error(QH_ERR_INVALID, "null buffer");
    if (in_stride < (long long)nblk * h->e.dsp_insize) return set_error(QH_ERR_INVALID, "stride shorter than nblk blocks");
    EgressFmt f{};
    if (int rc = make_egress(fmt, d_out, out_stride_bytes, (long long)nblk * h->e.dsp_outsize, &f)) return rc;
    if (rows_overlap(d_in, in_stride * 16, (long long)nblk * h->e.dsp_insize * 16, d_out, out_stride_bytes,
                     (long long)nblk * h->e.dsp_outsize * egress_frame_bytes(fmt), h->e.nch))
        return set_error(QH_ERR_INVALID, "qh_rxa_process_audio: the output rows overlap the input rows (in place is not supported)");
    h->e.eg = f;
    const int rc = h->e.process(d_in, in_stride, nullptr, 0, nblk);
    h->e.eg = EgressFmt{};
    return rc;
}

int qh_audio_pack(int device, void *stream, const double *d_src, long long src_stride, int nch, int n, const qh_audio_format *fmt,
                  void *d_dst, long long dst_stride_bytes)
{
    if (!d_src || nch <= 0 || n < 0) return set_error(QH_ERR_INVALID, "qh_audio_pack: bad arguments");
    if (qh_device_count() <= device || device < 0) return set_error(QH_ERR_NO_DEVICE, "no HIP device %d (libquiskhip has no CPU fallback)", device);
    EgressFmt f{};
    if (int rc = make_egress(fmt, d_dst, dst_stride_bytes, n, &f)) return rc;
    if (n == 0) return QH_OK;
    if (rows_overlap(d_src, src_stride * 16, (long long)n * 16, d_dst, dst_stride_bytes, (long long)n * egress_frame_bytes(fmt), nch))
        return set_error(QH_ERR_INVALID, "qh_audio_pack: the output rows overlap the input rows (in place is not supported)");
    QH_HIP(hipSetDevice(device));
    const long long per = ((long long)n + 255) / 256;
    hipLaunchKernelGGL(egress_pack_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)nch), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const double2 *>(d_src), src_stride, n, f);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

int qh_rxa_set_graph_replay(qh_rxa *h, int on)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    h->e.graph_on = on != 0;
    if (!on) { h->e.drop_graphs(); h->e.graph_key = Engine::GraphKey{}; }
    return QH_OK;
}
long long qh_rxa_graph_launches(const qh_rxa *h) { return h ? h->e.graph_launches : 0; }

int qh_rxa_set_band_tile(qh_rxa *h, int nfft)
{
    if (!h || (nfft != 0 && nfft != 4096 && nfft != 6144 && nfft != 8192)) return set_error(QH_ERR_INVALID, "qh_rxa_set_band_tile: 0 (default), 4096, 6144 or 8192");
    QH_RXA_LOCK(h);
    h->e.band_tile_pref = nfft;
    h->e.epoch++;                   // the next call picks the tile anew (pick_band_tile): a captured launch sequence runs the old one
    return QH_OK;
}
int qh_rxa_band_tile(const qh_rxa *h) { return h ? h->e.bnfft : 0; }

int Engine::process_replayed(const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk)
{
    // the resamplers (the output one; the input one of the rate ratios that are not 1, 2, 4, 8 or 16) keep a host-side phase and their
    // own ping-pong of delay lines per call, event timing records per call: all of them stay on the plain path.  (The input resampler was
    // missing here until a seeded walk through the WDSP names at 144 ksps found it: a sequence captured after a setter replayed the
    // other parity of its delay lines, tests/test_gpu_wdsp_names_fuzz.py.)
    if (rsmpin || rsmpout || timing || nblk <= 0) return process(d_in, in_stride, d_out, out_stride, nblk);
    const GraphKey key{d_in, d_out, in_stride, out_stride, nblk, epoch};
    if (!(key == graph_key)) { drop_graphs(); graph_key = key; graph_seen = false; }
    const unsigned before = flags();
    GraphSlot &slot = graph_slot[before];
    if (slot.exec) {
        QH_HIP(hipSetDevice(device));
        QH_HIP(hipGraphLaunch(slot.exec, stream));
        set_flags(slot.after);
        graph_launches++;
        return QH_OK;
    }
    if (!graph_seen) {
        // the first call under a new key uploads dirty parameters and grows buffers (synchronising): not capturable
        const int rc = process(d_in, in_stride, d_out, out_stride, nblk);
        graph_seen = rc == QH_OK;
        graph_key.epoch = epoch;        // buffers that this call grew are in place now
        return rc;
    }
    QH_HIP(hipSetDevice(device));
    if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        graph_on = false;
        return process(d_in, in_stride, d_out, out_stride, nblk);
    }
    const int rc = process(d_in, in_stride, d_out, out_stride, nblk);
    hipGraph_t g = nullptr;
    const hipError_t e_end = hipStreamEndCapture(stream, &g);
    bool ok = rc == QH_OK && e_end == hipSuccess && g && hipGraphInstantiate(&slot.exec, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (ok) {
        slot.after = flags();
        QH_HIP(hipGraphLaunch(slot.exec, stream));
        graph_launches++;
        return QH_OK;
    }
    // nothing ran: put the flags back, stop capturing for this engine and run the block the plain way
    (void)hipGetLastError();
    slot.exec = nullptr;
    set_flags(before);
    graph_on = false;
    return process(d_in, in_stride, d_out, out_stride, nblk);
}

// The same chain fed with wire-format samples: the front kernel decodes them in its load.
int qh_rxa_process_packed(qh_rxa *h, const void *d_src, long long src_bytes, const qh_iq_format *fmt, long long chan_stride,
                          double *d_out, long long out_stride, int nblk)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (!d_src || !d_out || !fmt) return set_error(QH_ERR_INVALID, "null buffer");
    if (out_stride < (long long)nblk * h->e.dsp_outsize) return set_error(QH_ERR_INVALID, "stride shorter than nblk blocks");
    PackedFmt pk;
    if (int rc = qh::make_packed_fmt(fmt, chan_stride, src_bytes, (long long)nblk * h->e.dsp_insize, h->e.nch, &pk)) return rc;
    if (rows_overlap(d_src, 0, src_bytes, d_out, out_stride * 16, (long long)nblk * h->e.dsp_outsize * 16, h->e.nch))
        return set_error(QH_ERR_INVALID, "qh_rxa_process_packed: the output rows overlap the packed source (in place is not supported)");
    h->e.pk_src = static_cast<const unsigned char *>(d_src);
    h->e.pk = pk;
    // process() wants an input pointer; the packed kernels never touch it
    const int rc = h->e.process(reinterpret_cast<const double *>(d_src), (long long)nblk * h->e.dsp_insize, d_out, out_stride, nblk);
    h->e.pk_src = nullptr;
    return rc;
}

// flush_rxa (wdsp/RXA.c:527-559): NCO phase, resampler ring and fircore delay lines back to zero
int qh_rxa_flush(qh_rxa *h)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    e.epoch++;
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipMemsetAsync(e.nco_phase, 0, (size_t)e.nch * sizeof(unsigned long long), e.stream));
    QH_HIP(hipMemsetAsync(e.nco_parked, 0, (size_t)e.nch * sizeof(unsigned long long), e.stream));
    if (e.rsmpout) if (int rc = qh_rat_reset(e.rsmpout)) return rc;        // flush_resample, wdsp/resample.c:159-165
    if (e.rsmpin) if (int rc = qh_rat_reset(e.rsmpin)) return rc;
    for (int i = 0; i < 2; i++) {
        if (e.hist_front[i]) QH_HIP(hipMemsetAsync(e.hist_front[i], 0, (size_t)e.nch * kHistFront * sizeof(double2), e.stream));
        QH_HIP(hipMemsetAsync(e.hist_nbp[i], 0, (size_t)e.nch * kHistBand * sizeof(double2), e.stream));
        QH_HIP(hipMemsetAsync(e.hist_bp1[i], 0, (size_t)e.nch * kHistBand * sizeof(double2), e.stream));
        if (e.demod_alloc) {
            QH_HIP(hipMemsetAsync(e.hist_de[i], 0, (size_t)e.nch * kHistBand * sizeof(double2), e.stream));
            QH_HIP(hipMemsetAsync(e.hist_aud[i], 0, (size_t)e.nch * kHistBand * sizeof(double2), e.stream));
        }
        for (int sid = 0; sid < 5; sid++)
            if (e.lhist[sid][i]) QH_HIP(hipMemsetAsync(e.lhist[sid][i], 0, (size_t)e.nch * kLongHist * sizeof(double2), e.stream));
    }
    if (e.demod_alloc) {                        // flush_wcpagc zeroes the ring (wcpAGC.c:154-159)
        for (int c = 0; c < e.nch; c++) {
            QH_HIP(hipMemsetAsync(e.agc_state[c].ring, 0, sizeof(e.agc_state[c].ring), e.stream));
            QH_HIP(hipMemsetAsync(e.agc_state[c].abs_ring, 0, sizeof(e.agc_state[c].abs_ring), e.stream));
            QH_HIP(hipMemsetAsync(&e.agc_state[c].ring_max, 0, sizeof(double), e.stream));
            if (e.cfg[(size_t)c].agc_stale) e.lists_dirty = true;
            e.cfg[(size_t)c].agc_stale = false;     // an empty ring and ring_max = 0: nothing stale (qh_agc_tiled.hpp)
        }
        if (e.agc_lring) {
            QH_HIP(hipMemsetAsync(e.agc_lring, 0, (size_t)e.nch * kAgcLongRing * sizeof(double2), e.stream));
            QH_HIP(hipMemsetAsync(e.agc_labs, 0, (size_t)e.nch * kAgcLongRing * sizeof(double), e.stream));
        }
    }
    for (ChanCfg &c : e.cfg) { c.lms[0].flush = c.lms[1].flush = true; c.emnr_flush = true; c.snba_flush = true; c.snb_flush = true; }    // flush_anf / flush_anr / flush_emnr, RXA.c:541-543
    if (e.amsq_state) QH_HIP(hipMemsetAsync(e.amsq_state, 0, (size_t)e.nch * sizeof(AmsqState), e.stream));     // flush_amsq
    if (e.ap_state) QH_HIP(hipMemsetAsync(e.ap_state, 0, (size_t)e.nch * kApW * sizeof(double), e.stream));    // flush_cbl / _speak / _mpeak, RXA.c:553-555
    if (e.ssql_state) hipLaunchKernelGGL(ssql_flush_kernel, dim3((unsigned)e.nch), dim3(64), 0, e.stream, e.ssql_state);    // flush_ssql, RXA.c:556
    if (e.demod_alloc) {                        // flush_amd / flush_fmd / flush_snotch
        QH_HIP(hipMemsetAsync(e.am_state, 0, (size_t)e.nch * sizeof(AmState), e.stream));
        QH_HIP(hipMemsetAsync(e.pll_state, 0, (size_t)e.nch * sizeof(PllState), e.stream));
        QH_HIP(hipMemsetAsync(e.fm_pll_state, 0, (size_t)e.nch * sizeof(PllState), e.stream));
        QH_HIP(hipMemsetAsync(e.sn_state, 0, (size_t)e.nch * sizeof(SnotchState), e.stream));
    }
    return QH_OK;
}

// Meters (wdsp/meter.c): enable != 0 makes later process calls maintain the ADC, S and AGC meters.
int qh_rxa_enable_meters(qh_rxa *h, int enable)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    h->e.meters_on = enable != 0;
    h->e.epoch++;                   // the meter launches join / leave the sequence
    return QH_OK;
}

// GetRXAMeter (wdsp/meter.c:133-142); mt as wdsp/RXA.h:47-57: 0 S_PK, 1 S_AV, 2 ADC_PK, 3 ADC_AV, 4 AGC_GAIN, 5 AGC_PK, 6 AGC_AV
int qh_rxa_GetRXAMeter(qh_rxa *h, int ch, int mt, double *value)
{
    if (!h || !value) return set_error(QH_ERR_INVALID, "null argument");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (ch < 0 || ch >= e.nch || mt < 0 || mt > 6) return set_error(QH_ERR_INVALID, "channel or meter index out of range");
    if (!e.meters_on || !e.m_adc) { *value = -400.0; return QH_OK; }             // flush_meter's initial reading
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipStreamSynchronize(e.stream));
    MeterState st;
    const MeterState *src = mt <= 1 ? e.m_s : mt <= 3 ? e.m_adc : e.m_agc;
    QH_HIP(hipMemcpy(&st, src + ch, sizeof(st), hipMemcpyDeviceToHost));
    if (mt == 4) {
        double g = 0.0;
        // RXA_AGC_GAIN: xwcpagc's `gain` (wcpAGC.c:334), which only the modes 1-5 write; 0 from create_wcpagc's calloc until then
        if (e.agc_state) QH_HIP(hipMemcpy(&g, &e.agc_state[ch].gain, sizeof(double), hipMemcpyDeviceToHost));
        const double v = g + 1.0e-40;
        unsigned long long N; std::memcpy(&N, &v, 8);
        const int ex = (int)((N >> 52) & 2047) - 1023, m = (int)((N >> 41) & 2047);
        *value = 20.0 * 0.301029995663981 * ((double)ex + std::log2(1.0 + (double)m / 2048.0));
        return QH_OK;
    }
    *value = (mt == 0 || mt == 2 || mt == 5) ? st.res_pk : st.res_av;
    return QH_OK;
}

// Diagnostics of the time-tiled FM loop: tiles whose speculative warm-up had not converged and were re-run in order.
long long qh_rxa_pll_repairs(qh_rxa *h)
{
    if (!h || !h->e.pll_nfixed) return 0;
    int v = 0;
    if (hipSetDevice(h->e.device) != hipSuccess || hipStreamSynchronize(h->e.stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, h->e.pll_nfixed, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

// Diagnostics: check_only >= 0 sets the verify pass to count-only (1) or repair (0); then copies up to `max` doubles of
// channel ch's per-tile loop states of the last call ([tile][kPllEndsW]: pt, fil_out, omega where the warm-up ended / the tile ended).
int qh_rxa_debug_pll(qh_rxa *h, int check_only, int ch, double *out, int max)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (check_only >= 0) e.pll_check_only = check_only;
    if (!out || max <= 0 || !e.pll_ends) return 0;
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipStreamSynchronize(e.stream));
    long long n = e.pll_ends_cap * kPllEndsW;
    if (n > max) n = max;
    QH_HIP(hipMemcpy(out, e.pll_ends + (long long)ch * e.pll_ends_cap * kPllEndsW, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return (int)n;
}

// Diagnostics: the lanes' states of the last time-tiled wcpAGC call, list slot `slot`: [tile][kAgcEndsW]
int qh_rxa_debug_agc_ends(qh_rxa *h, int slot, double *out, int max)
{
    if (!h || !out || max <= 0 || !h->e.agc_ends) return 0;
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipStreamSynchronize(e.stream));
    // [tile][8] boundary states (what the run-jumping pass found), then [tile][8] the states the exact tiles ended in
    long long n = e.agc_ends_cap * kAgcEndsW;
    if (2 * n > max) n = max / 2;
    QH_HIP(hipMemcpy(out, e.agc_ends + (long long)slot * e.agc_ends_cap * kAgcEndsW, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    QH_HIP(hipMemcpy(out + n, e.agc_ends + ((long long)e.nch + slot) * e.agc_ends_cap * kAgcEndsW, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    n *= 2;
    return (int)n;
}

// tiles of the time-tiled wcpAGC that the verify pass re-ran in order, over all calls so far
long long qh_rxa_agc_repairs(qh_rxa *h)
{
    if (!h || !h->e.agc_nfixed) return 0;
    QH_RXA_LOCK(h);
    int v = 0;
    if (hipSetDevice(h->e.device) != hipSuccess || hipStreamSynchronize(h->e.stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, h->e.agc_nfixed, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

// super-segments of the AGC boundary pass that were walked again (their warm-up had not ended on the true trajectory), over all calls
#ifdef QH_AGC_COUNT
extern "C" int qh_dbg_agc_counts(unsigned long long *out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(qh::g_agc_count), 20 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[20] = { 0 }; if (hipMemcpyToSymbol(HIP_SYMBOL(qh::g_agc_count), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif
long long qh_rxa_agc_segments_rerun(qh_rxa *h)
{
    if (!h || !h->e.agc_nfixed) return 0;
    QH_RXA_LOCK(h);
    int v = 0;
    if (hipSetDevice(h->e.device) != hipSuccess || hipStreamSynchronize(h->e.stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, h->e.agc_nfixed + 1, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

// channels whose xwcpagc ran in time tiles in the last call (the others, if any: one wavefront per channel)
int qh_rxa_agc_tiled_channels(qh_rxa *h)
{
    if (!h) return 0;
    QH_RXA_LOCK(h);
    return h->e.agc_last_tiled;
}

// Diagnostics: which form of the wcpAGC loop runs (0: time tiles for long calls, else 64 samples per step of the wavefront; 1: sample by
// sample; 2: 64 samples per step whatever the call length).  Same state; 1 and 2 give the same bits, 0 the same to rounding.
int qh_rxa_debug_agc(qh_rxa *h, int form)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (h->e.agc_form != form) { h->e.agc_form = form; h->e.drop_graphs(); h->e.epoch++; }
    return QH_OK;
}

int qh_rxa_synchronize(qh_rxa *h)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    QH_HIP(hipSetDevice(h->e.device));
    QH_HIP(hipStreamSynchronize(h->e.stream));
    return QH_OK;
}

int qh_rxa_process_host(qh_rxa *h, const double *h_in, long long in_stride, double *h_out, long long out_stride, int nblk)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (!h_in || !h_out) return set_error(QH_ERR_INVALID, "null buffer");
    Engine &e = h->e;
    QH_HIP(hipSetDevice(e.device));
    const long long n_in = (long long)nblk * e.dsp_insize, n_out = (long long)nblk * e.dsp_outsize;
    double2 *din = nullptr, *dout = nullptr;
    QH_HIP(dev_alloc(&din, (size_t)e.nch * (size_t)n_in));
    QH_HIP(dev_alloc(&dout, (size_t)e.nch * (size_t)n_out));
    int rc = QH_OK;
    hipError_t err = hipMemcpy2DAsync(din, (size_t)n_in * sizeof(double2), h_in, (size_t)in_stride * sizeof(double2),
                                      (size_t)n_in * sizeof(double2), (size_t)e.nch, hipMemcpyHostToDevice, e.stream);
    if (err == hipSuccess) {
        rc = e.process(reinterpret_cast<const double *>(din), n_in, reinterpret_cast<double *>(dout), n_out, nblk);
        if (rc == QH_OK)
            err = hipMemcpy2DAsync(h_out, (size_t)out_stride * sizeof(double2), dout, (size_t)n_out * sizeof(double2),
                                   (size_t)n_out * sizeof(double2), (size_t)e.nch, hipMemcpyDeviceToHost, e.stream);
    }
    hipError_t err2 = hipStreamSynchronize(e.stream);
    (void)hipFree(din); (void)hipFree(dout);
    if (rc != QH_OK) return rc;
    if (err != hipSuccess) return set_error(QH_ERR_HIP, "copy failed: %s", hipGetErrorString(err));
    if (err2 != hipSuccess) return set_error(QH_ERR_HIP, "synchronize failed: %s", hipGetErrorString(err2));
    return QH_OK;
}

int qh_rxa_process_packed_host(qh_rxa *h, const void *h_src, long long src_bytes, const qh_iq_format *fmt, long long chan_stride,
                               double *h_out, long long out_stride, int nblk)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (!h_src || !h_out || src_bytes <= 0) return set_error(QH_ERR_INVALID, "null buffer");
    Engine &e = h->e;
    QH_HIP(hipSetDevice(e.device));
    const long long n_out = (long long)nblk * e.dsp_outsize;
    unsigned char *dsrc = nullptr;
    double2 *dout = nullptr;
    QH_HIP(dev_alloc(&dsrc, (size_t)src_bytes));
    if (dev_alloc(&dout, (size_t)e.nch * (size_t)n_out) != hipSuccess) { (void)hipFree(dsrc); return set_error(QH_ERR_HIP, "hipMalloc failed"); }
    int rc = QH_OK;
    hipError_t err = hipMemcpyAsync(dsrc, h_src, (size_t)src_bytes, hipMemcpyHostToDevice, e.stream);
    if (err == hipSuccess) {
        rc = qh_rxa_process_packed(h, dsrc, src_bytes, fmt, chan_stride, reinterpret_cast<double *>(dout), n_out, nblk);
        if (rc == QH_OK)
            err = hipMemcpy2DAsync(h_out, (size_t)out_stride * sizeof(double2), dout, (size_t)n_out * sizeof(double2),
                                   (size_t)n_out * sizeof(double2), (size_t)e.nch, hipMemcpyDeviceToHost, e.stream);
    }
    hipError_t err2 = hipStreamSynchronize(e.stream);
    (void)hipFree(dsrc); (void)hipFree(dout);
    if (rc != QH_OK) return rc;
    if (err != hipSuccess) return set_error(QH_ERR_HIP, "copy failed: %s", hipGetErrorString(err));
    if (err2 != hipSuccess) return set_error(QH_ERR_HIP, "synchronize failed: %s", hipGetErrorString(err2));
    return QH_OK;
}

int qh_rxa_enable_timing(qh_rxa *h, int enable)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    h->e.timing = enable != 0;
    return QH_OK;
}

int qh_rxa_timing(qh_rxa *h, double *ms, int n)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipStreamSynchronize(e.stream));
    double acc[3] = { 0, 0, 0 };
    for (int i = 0; i + 1 < e.ev_used; i++) {
        float t = 0;
        QH_HIP(hipEventElapsedTime(&t, e.ev[(size_t)i], e.ev[(size_t)i + 1]));
        int cat = e.ev_cat[(size_t)i];
        if (cat >= 0 && cat < 3) acc[cat] += t;
    }
    for (int k = 0; k < 3; k++) { e.last_ms[k] = acc[k]; if (k < n) ms[k] = acc[k]; }
    return n < 3 ? n : 3;
}

}  // extern "C"
