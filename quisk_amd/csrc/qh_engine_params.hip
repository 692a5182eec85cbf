// qh_engine_params.hip -- the parameter side of the RXA engine (qh_engine.hpp): what runs when a setter has marked something dirty or a
// stage is first used -- filter designs, masks, channel lists, per-channel parameter rows, first-use allocation, buffer growth, flush.
// Host code only: the few kernels that rewrite state for new parameters (oscillator retune, front masks, SSQL flush) are launched through
// Engine::launch_* of qh_engine.hip, so this unit's object holds no device code.  No ABI function lives here (qh_rxa_api.hip).
#include "qh_engine.hpp"
#include <new>

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
    if (disp_fed) (void)hipEventDestroy(disp_fed);
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

int check_rates(const char *who, int dsp_size, int in_rate, int dsp_rate, int out_rate, int *D)
{
    if (dsp_size <= 0 || (dsp_size & (dsp_size - 1)) || in_rate <= 0 || dsp_rate <= 0) return set_error(QH_ERR_INVALID, "%s: bad arguments", who);
    if (out_rate <= 0 || (out_rate % dsp_rate && dsp_rate % out_rate) || (out_rate < dsp_rate && dsp_size % (dsp_rate / out_rate)))
        return set_error(QH_ERR_UNSUPPORTED, "out_rate must be an integer multiple or fraction of dsp_rate (wdsp/channel.c:47-52)");
    // in_rate / dsp_rate 1, 2, 4, 8, 16: the overlap-save front stage.  Any other whole ratio, up or down (3, 5, 6 ...; 1/2,
    // 1/4 ...): xshift as a pointwise pass + the polyphase form of xresample (wdsp/resample.c:35-157) -- D = 0 marks it.  The
    // reference sizes its blocks with integer divisions of the two rates (pre_main_build, wdsp/channel.c:39-42): a ratio that is
    // not whole one way or the other does not give it consistent block sizes, and is refused here.
    *D = (in_rate % dsp_rate) ? 0 : in_rate / dsp_rate;
    if (*D != 1 && *D != 2 && *D != 4 && *D != 8 && *D != 16) *D = 0;
    if (*D == 0 && !((in_rate > dsp_rate && in_rate % dsp_rate == 0) ||
                     (in_rate < dsp_rate && dsp_rate % in_rate == 0 && dsp_size % (dsp_rate / in_rate) == 0)))
        // (a CPU test of the reference's arithmetic, test_rates_that_are_whole_in_neither_direction_recycle_stale_buffer_tails, shows what it
        // does with 96 k -> 64 k -> 48 k: every block's tail is what the block before left in the buffer)
        return set_error(QH_ERR_UNSUPPORTED, "in_rate / dsp_rate must be a whole number or the reciprocal of one (wdsp/channel.c:39-42)");
    return QH_OK;
}

bool eqp_profile_tie(const std::vector<double> &F, const std::vector<double> &G, double rate)
{
    for (size_t i = 1; i < F.size(); i++)
        for (size_t j = i + 1; j < F.size(); j++) {
            const double a = std::min(1.0, std::max(0.0, 2.0 * F[i] / rate)), b = std::min(1.0, std::max(0.0, 2.0 * F[j] / rate));
            if (a == b && G[i] != G[j]) return true;
        }
    return false;
}

// xresample in (wdsp/RXA.c:48-57) for in_rate / dsp_rate: D > 1 the overlap-save tile stage and its delay line, zeroed; D = 0 the polyphase
// rsmpin; D = 1 neither (RXAResCheck, RXA.c:789-798).  What an earlier ratio had made and this one does not use is given back.
int Engine::front_build()
{
    // pre_main_build, wdsp/channel.c:39-42
    dsp_insize = D > 0 ? dsp_size * D : (int)((long long)dsp_size * in_rate / dsp_rate);
    if (rsmpin) { qh_rat_destroy(rsmpin); rsmpin = nullptr; }
    if (D == 0) {
        // create_resample(..., in_rate, dsp_rate, 0.0, 0, 1.0), wdsp/RXA.c:48-57
        const ResamplerDesign rd = design_resampler(in_rate, dsp_rate, 0.0, 0, 1.0);
        std::vector<double> taps(rd.h);
        for (double &v : taps) v /= (double)rd.L;           // qh_rat applies the gain `interp` itself (quisk_cInterpDecim's convention)
        rsmpin = qh_rat_create(device, nch, taps.data(), rd.ncoef, rd.L, rd.M, QH_F64, stream);
        if (!rsmpin) return QH_ERR_HIP;
    }
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
        std::vector<cd> twi = fft_twiddle_table(kNfft / front_fold);
        if (int rc = alloc(tw_inv_front, (long long)twi.size())) return rc;
        if (int rc = upload(tw_inv_front, twi, stream)) return rc;
        for (double2 *&h : hist_front) if (int rc = alloc(h, (long long)nch * kHistFront, true)) return rc;
    } else {
        front_fold = front_pick = 1; front_ntaps = front_P = front_L = 0;
        release(mask_front); release(lane_rot); release(front_taps); release(retune_list); release(retune_law); release(tw_inv_front);
        for (double2 *&h : hist_front) release(h);
    }
    return QH_OK;
}

// xresample out (wdsp/RXA.c:474-484) for dsp_rate / out_rate; none when the two are equal (RXAResCheck, RXA.c:789-798)
int Engine::out_build()
{
    dsp_outsize = out_rate >= dsp_rate ? dsp_size * (out_rate / dsp_rate) : dsp_size / (dsp_rate / out_rate);    // channel.c:44-47
    if (rsmpout) { qh_rat_destroy(rsmpout); rsmpout = nullptr; }
    if (out_rate != dsp_rate) {
        // create_resample(..., dsp_rate, out_rate, 0.0, 0, 1.0), wdsp/RXA.c:474-484; the polyphase loop of xresample
        // (resample.c:120-157) is quisk_cInterpDecim's with the gain already in the taps
        const ResamplerDesign rd = design_resampler(dsp_rate, out_rate, 0.0, 0, 1.0);
        std::vector<double> taps(rd.h);
        for (double &v : taps) v /= (double)rd.L;
        rsmpout = qh_rat_create(device, nch, taps.data(), rd.ncoef, rd.L, rd.M, QH_F64, stream);
        if (!rsmpout) return QH_ERR_HIP;
    }
    return QH_OK;
}

int Engine::init()
{
    QH_HIP(hipSetDevice(device));
    if (!stream) { QH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); own_stream = true; }
    cfg.assign((size_t)nch, ChanCfg());
    for (ChanCfg &c : cfg) c.eqp_nc = c.fm_nc_de = c.fm_nc_aud = std::max(2048, dsp_size);     // create_eqp's nc, RXA.c:265; create_fmd's, RXA.c:209,211
    wide.snba_tune_h.assign((size_t)nch, SnbaTune{ 64, 2, 10, 2, 2, 0, 8.0, 20.0, 0.5 });         // create_snba's arguments, RXA.c:183-202
    // the fircore stages: the FM pair holds a mask row per distinct design among its channels (one row to begin with), xfmsq's noise
    // filter one design for its channels, the others one per channel
    for (int s = 0; s < FC_COUNT; s++) {
        fc[s].mask_stride = s == FC_DE || s == FC_AUD || s == FC_FQ ? 0 : kBandNfftMax;
        fc[s].by_design = s == FC_DE || s == FC_AUD;
        fc[s].chan.assign((size_t)nch, Fircore::Chan());
    }
    fc[FC_NBP].dirty = &ChanCfg::Work::nbp_dirty; fc[FC_BP1].dirty = &ChanCfg::Work::bp1_dirty; fc[FC_SNB].dirty = &ChanCfg::Work::snb_dirty;
    fc[FC_FQ].can_long = fc[FC_EQP].can_long = false;

    std::vector<cd> tw = fft_twiddle_table(kNfft);
    if (int rc = alloc(tw4096, (long long)tw.size())) return rc;
    if (int rc = upload(tw4096, tw, stream)) return rc;
    tw = fft_twiddle_table(kBandNfftMax);
    if (int rc = alloc(tw8192, (long long)tw.size())) return rc;
    if (int rc = upload(tw8192, tw, stream)) return rc;

    if (int rc = front_build()) return rc;
    if (int rc = out_build()) return rc;
    if (int rc = fc_alloc(fc[FC_NBP])) return rc;
    if (int rc = fc_alloc(fc[FC_BP1])) return rc;
    if (int rc = alloc(nco_phase, nch, true)) return rc;
    if (int rc = alloc(nco_dphase, nch, true)) return rc;
    if (int rc = alloc(nco_parked, nch, true)) return rc;
    if (int rc = alloc(nco_step, nch)) return rc;
    if (int rc = alloc(epi, nch)) return rc;

    if (int rc = tile_lds_limits()) return rc;
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
    // nbp0's and bp1's designs: what they are made from, and the last one made (its impulse response and one-tile mask), which the next
    // channel with the same settings takes over.  notch: nbp0 with its notch database, which is the channel's own -- never taken over.
    struct BandSet {
        int run, nc, wintype, mp, notch; double flow, fhigh, gain;
        bool operator==(const BandSet &o) const
        { return run == o.run && nc == o.nc && wintype == o.wintype && mp == o.mp && notch == o.notch && flow == o.flow && fhigh == o.fhigh && gain == o.gain; }
    };
    struct BandLast { bool any = false; BandSet set; std::vector<cd> h, mask; } last_nbp, last_bp1;
    auto design_band = [&](Fircore &f, const ChanCfg &c, int ch, const BandSet &d, BandLast &last) -> int {
        if (!(last.any && !d.notch && last.set == d)) {
            std::vector<cd> &h = last.h;
            if (d.run) {
                // calc_nbp_impulse, wdsp/nbp.c:221-238; bp1: wdsp/bandpass.c:302
                const double scale = d.gain / (double)(2 * dsp_size);
                h = d.notch ? notched(c, d.nc, d.flow, d.fhigh, scale) : fir_bandpass(d.nc, d.flow, d.fhigh, (double)dsp_rate, d.wintype, 1, scale);
                if (d.mp) h = mp_imp(h, 16, 0);             // calc_fircore, wdsp/firmin.c:327-328
                // the reference's unnormalised inverse FFT of 2*size points restores the 1/(2*size)
                for (auto &v : h) v *= (double)(2 * dsp_size);
            } else h.assign(1, cd(1.0, 0.0));               // identity when the filter is off
            last.mask.clear(); last.set = d; last.any = true;
        }
        return put_taps(f, ch, last.h, last.mask);
    };
    // Oscillator changes (SetRXAShiftFreq / SetRXAShiftRun).  With a front FIR stage (D > 1) the oscillator sits behind
    // the filter: first the stored raw history of every changed channel is re-expressed for its new phase law (the kernel
    // reads the old law from the device arrays, so it goes first), then the arrays are updated, then the channel's
    // modulated mask and phasor tables are rebuilt.
    std::vector<int> nco_list;
    if (D > 1) {
        std::vector<unsigned long long> law;
        for (int ch = 0; ch < nch; ch++) {
            const ChanCfg &c = cfg[(size_t)ch];
            if (!c.w.nco_dirty) continue;
            nco_list.push_back(ch);
            const bool flip = (c.shift_run != 0) != (c.w.shift_on_device != 0);
            law.push_back(flip ? (c.shift_run ? 2ull : 1ull) : 0ull);
            law.push_back(c.shift_run ? turns_fx(c.shift_freq, (double)in_rate) : 0ull);
        }
        if (!nco_list.empty()) {
            QH_HIP(hipMemcpyAsync(retune_list, nco_list.data(), nco_list.size() * sizeof(int), hipMemcpyHostToDevice, stream));
            QH_HIP(hipMemcpyAsync(retune_law, law.data(), law.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
            launch_nco_retune((int)nco_list.size());
            QH_HIP(hipStreamSynchronize(stream));           // the host vectors die with this scope
        }
    }
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (c.w.nco_dirty) {
            if ((c.shift_run != 0) != (c.w.shift_on_device != 0)) {
                launch_nco_park(ch, c.shift_run ? 1 : 0);
                c.w.shift_on_device = c.shift_run ? 1 : 0;
            }
            // calc_shift, wdsp/shift.c:29-34: delta = 2*pi*shift/rate per input sample
            if (int rc = put_row(nco_dphase, ch, c.shift_run ? turns_fx(c.shift_freq, (double)in_rate) : 0ull)) return rc;
            c.w.nco_dirty = false;
        }
        if (c.w.epi_dirty) {
            // xwcpagc mode 0 (wcpAGC.c:167-175) then xpanel (patchpanel.c:55-101) as one 2x2 real matrix
            // (with a position-1 anf / anr / bp1 behind it the gain is applied at the AGC's own spot instead: fix_before)
            const double g = (c.agc_run && c.agc_mode == 0 && !c.fix_before()) ? c.agc_fixed : 1.0;
            const double g2 = g * g;            // the agc meter reads |g z|^2 off the signal ahead of the output matrix
            if (m_g2) if (int rc = put_row(m_g2, ch, g2, false)) return rc;
            if (tap_gain) if (int rc = put_row(tap_gain, ch, g, false)) return rc;      // the siphon reads g z there too
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
            c.w.epi_dirty = false;
        }
        if (c.w.nbp_dirty) c.w.snb_dirty = true;        // bpsnba's nbp shares window, auto-increase and the notch database with nbp0 (nc and mp are its own)
        if (c.w.snb_dirty && c.snba_run && fc[FC_SNB].mask) if (int rc = snb_mask(c, ch)) return rc;
        if (c.w.snb_flush && fc[FC_SNB].hist[0]) if (int rc = zero_rows(fc[FC_SNB], ch)) return rc;         // setNc_fircore zeroes the delay line
        c.w.snb_flush = false;
        if (c.w.nbp_dirty) {
            if (int rc = design_band(fc[FC_NBP], c, ch, { c.nbp_run, c.nbp_nc, c.nbp_wintype, c.nbp_mp, c.fnfrun, c.nbp_flow, c.nbp_fhigh, c.nbp_gain }, last_nbp)) return rc;
            c.w.nbp_dirty = false;
        }
        if (c.w.bp1_dirty) {
            if (int rc = design_band(fc[FC_BP1], c, ch, { c.bp1_run, c.bp1_nc, c.bp1_wintype, c.bp1_mp, 0, c.bp1_flow, c.bp1_fhigh, c.bp1_gain }, last_bp1)) return rc;
            c.w.bp1_dirty = false;
            lists_dirty = true;             // the channel pairs of the real bp1 filters follow the designs
        }
        if (c.w.nbp_flush) {      // setNc_fircore re-plans and so zeroes the delay line
            if (int rc = zero_rows(fc[FC_NBP], ch)) return rc;
            c.w.nbp_flush = false;
        }
        if (c.w.bp1_flush) {      // flush_bandpass on off->on (RXA.c:825) and setNc_fircore
            if (int rc = zero_rows(fc[FC_BP1], ch)) return rc;
            c.w.bp1_flush = false;
        }
    }
    if (!nco_list.empty())      // retune_list still holds the channels; the new dphase values are in place
        launch_front_masks((int)nco_list.size());
    return QH_OK;
}

// calc_nbp_impulse with the notches, wdsp/nbp.c:221-232: bands in absolute frequency, filter in baseband; nc: the stage's own (nbp0's or bpsnba's)
std::vector<cd> Engine::notched(const ChanCfg &c, int nc, double f_low, double f_high, double scale) const
{
    const double offset = c.ndb_tunefreq + c.ndb_shift;
    const double minwidth = (c.nbp_wintype == 1 ? 2200.0 : 1600.0) / (nc / 256) * ((double)dsp_rate / 48000);
    std::vector<std::pair<double, double>> bands = make_nbp(c.notches, minwidth, c.autoincr, f_low + offset, f_high + offset, nullptr);
    for (auto &b : bands) { b.first -= offset; b.second -= offset; }
    return fir_mbandpass(nc, bands, (double)dsp_rate, scale, c.nbp_wintype);
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
    if (fc[FC_SNB].parts > 1) if (int rc = long_stage_alloc(fc[FC_SNB])) return rc;
    std::vector<cd> h = run_notches ? notched(c, c.snb_nc, f_low, f_high, scale) : fir_bandpass(c.snb_nc, f_low, f_high, (double)dsp_rate, c.nbp_wintype, 1, scale);
    if (c.snb_mp) h = mp_imp(h, 16, 0);
    for (auto &v : h) v *= (double)(2 * dsp_size);
    std::vector<cd> m;
    if (int rc = put_taps(fc[FC_SNB], ch, h, m)) return rc;
    c.w.snb_dirty = false;
    return QH_OK;
}

// The taps h of row `row` of a fircore stage's masks (a channel's row, or row 0 of a shared mask) onto the device: the partitions' masks
// when the stage runs its long form, and the one-tile mask (the bnfft bins of the tile in use; of the first kLongPart taps, and not used,
// in the long form).  m: that mask, made here when the caller passes it empty and left to it for the next row of the same design.
int Engine::put_taps(Fircore &f, int row, const std::vector<cd> &h, std::vector<cd> &m)
{
    if (f.parts > 1) if (int rc = long_masks_upload(f, row, h)) return rc;
    if (m.empty()) m = band_mask((int)h.size() > kLongPart ? std::vector<cd>(h.begin(), h.begin() + kLongPart) : h);
    QH_HIP(hipMemcpyAsync(f.mask + (size_t)row * (size_t)f.mask_stride, m.data(), (size_t)bnfft * sizeof(cd), hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));       // the host vectors die with the callers' scopes
    return QH_OK;
}

// A fircore stage's device rows: its masks and its delay lines, zeroed; every channel's line lies in the half that is current
int Engine::fc_alloc(Fircore &f)
{
    if (int rc = alloc(f.mask, f.mask_rows(nch) * kBandNfftMax)) return rc;
    if (f.carried) { f.carried = false; return QH_OK; }
    for (double2 *&h : f.hist) if (int rc = alloc(h, (long long)nch * kHistBand, true)) return rc;
    for (Fircore::Chan &r : f.chan) { r.listed = false; r.at = f.cur; }
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
    // the fused taps' tables (qh_osfir.hpp): a lane's weight (1 - m) m^(lanes - 1 - t) for tiles of 256 and of 384 lanes, and the peak's
    // decay over k blocks mp^(dsp_size k) -- a tile of at most 6144 samples meets 6144 / 64 + 1 blocks of 64 or more
    std::vector<double> w((size_t)kMeterTabDoubles), g2((size_t)nch);
    const double ln_m = -1.0 / (rate * 0.100);
    for (int t = 0; t < 256; t++) w[(size_t)t] = (1.0 - m_prm.mult_average) * std::exp(ln_m * (double)(255 - t));
    for (int t = 0; t < 384; t++) w[(size_t)(kMeterW384 + t)] = (1.0 - m_prm.mult_average) * std::exp(ln_m * (double)(383 - t));
    for (int k = 0; k < kMeterPkLen; k++) w[(size_t)(kMeterPk + k)] = std::exp(ln_m * (double)dsp_size * (double)k);
    for (int ch = 0; ch < nch; ch++) {
        const ChanCfg &c = cfg[(size_t)ch];
        g2[(size_t)ch] = (c.agc_run && c.agc_mode == 0 && !c.fix_before()) ? c.agc_fixed * c.agc_fixed : 1.0;
    }
    if (int rc = alloc(m_w, kMeterTabDoubles)) return rc;
    if (int rc = alloc(m_g2, nch)) return rc;
    QH_HIP(hipMemcpyAsync(m_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, stream));
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
    if (int rc = fc_alloc(fc[FC_DE])) return rc;
    if (int rc = fc_alloc(fc[FC_AUD])) return rc;
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
    for (ChanCfg &c : cfg) c.w.demod_dirty = true;
    return QH_OK;
}

// Every channel list from the channels' settings (host side: h[id]), with their counts
void Engine::build_lists(std::vector<int> (&h)[L_COUNT])
{
    std::vector<int> stale_cur, stale_other;
    int sam0 = 0;
    ssql_lists.clear(); fq_lists.clear(); tap_lists.clear(); gen_lists.clear(); lms_long_lists.clear();
    for (unsigned &ks : lms_long_Ks) ks = 0;
    for (int ch = 0; ch < nch; ch++) {
        const ChanCfg &c = cfg[(size_t)ch];
        if (c.sender_run) tap_lists.h[0].push_back(ch);
        if (c.gen_run) gen_lists.h[0].push_back(ch);
        if (c.sip_run) tap_lists.h[c.bp1_run ? 2 : 1].push_back(ch);          // where the agc meter finds the channel (L_PLAIN / L_BP1)
        if (c.amsq_run) h[L_AMSQ].push_back(ch);
        if (c.snba_run) h[L_SNBA].push_back(ch);
        if (c.snb_pos() >= 0) h[L_SNB + c.snb_pos()].push_back(ch);
        const int at_agc = (c.bp1_run && !c.bp1_pos) ? 1 : 0;       // the buffer the channel is in when xwcpagc runs
        if (c.emnr_run) h[L_EMNR + (c.emnr_pos ? 1 + at_agc : 0)].push_back(ch);
        for (int f = 0; f < 2; f++) {
            if (!c.lms[f].run) continue;
            const int k = 3 * f + (c.lms[f].position ? 1 + at_agc : 0);
            if (!lms_long_form(c.lms[f])) { h[L_LMS + k].push_back(ch); continue; }
            lms_long_lists.h[k].push_back(ch);
            lms_long_Ks[k] |= (unsigned)lms_long_K(c.lms[f].taps);          // K is a power of two: its own bit
        }
        if (c.bp1_run) h[L_BP1P + (c.bp1_pos ? 1 : 0)].push_back(ch);
        if (c.fix_before()) h[L_FIX + at_agc].push_back(ch);
        if (c.ap_on()) h[L_AP + (c.bp1_run ? 1 : 0)].push_back(ch);        // where the channel is behind bp1 at either position
        if (c.ssql_on()) ssql_lists.h[c.bp1_run ? 1 : 0].push_back(ch);
        if (c.fmd_run && c.lim_run) h[L_LIM].push_back(ch);
        if (c.fmd_run && c.fmsq_run) fq_lists.h[0].push_back(ch);
        if (c.amd_run && c.amd_mode == 0) h[L_AM].push_back(ch);
        // SAM channels with sbmode 0 (no all-pass chains) first
        if (c.amd_run && c.amd_mode == 1) { if (c.sbmode == 0) h[L_SAM].insert(h[L_SAM].begin() + sam0++, ch); else h[L_SAM].push_back(ch); }
        if (c.fmd_run) h[L_FM].push_back(ch); else { h[L_REST].push_back(ch); h[c.bp1_run ? L_RB : L_USB].push_back(ch); }
        h[c.bp1_run ? L_BP1 : L_PLAIN].push_back(ch);
        // xwcpagc sits between the two bp1 positions (RXA.c:581-586): a position-1 channel is still in `cur` there; channels whose
        // attack window moved in mid-stream go last
        if (c.agc_run && c.agc_mode != 0) (at_agc ? (c.w.agc_stale ? stale_other : h[L_AGC_OTHER]) : (c.w.agc_stale ? stale_cur : h[L_AGC_CUR])).push_back(ch);
    }
    n_sam0 = sam0;
    n_agc_cur_stale = (int)stale_cur.size(); n_agc_other_stale = (int)stale_other.size();
    h[L_AGC_CUR].insert(h[L_AGC_CUR].end(), stale_cur.begin(), stale_cur.end());
    h[L_AGC_OTHER].insert(h[L_AGC_OTHER].end(), stale_other.begin(), stale_other.end());
    // partners: neighbours in the list, ordered so that equal designs are neighbours; a channel left over is its own partner
    auto bp1_real = [&](int ch) { const ChanCfg &c = cfg[(size_t)ch]; return c.bp1_run && c.bp1_flow == -c.bp1_fhigh && !c.bp1_mp; };
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
    // the FM de-emphasis stage: by design row, which is by what the row is designed from (fm_filters); one design leaves the list's order
    {
        auto de_key = [&](int ch) { const ChanCfg &c = cfg[(size_t)ch]; return std::make_tuple(c.fm_nc_de, c.fm_mp_de, c.fm_f_low, c.fm_f_high); };
        std::vector<int> fm(h[L_FM]);
        std::stable_sort(fm.begin(), fm.end(), [&](int x, int y) { return de_key(x) < de_key(y); });
        for (size_t i = 0; i < fm.size();) {
            const bool two = i + 1 < fm.size() && de_key(fm[i]) == de_key(fm[i + 1]);
            h[L_PAIRS_FM].push_back(fm[i]); h[L_PAIRS_FM].push_back(two ? fm[i + 1] : fm[i]);
            i += two ? 2 : 1;
        }
    }
    h[L_PAIRS_AM] = bp1_pairs(h[L_AM]);
    h[L_PAIRS_SAM] = bp1_pairs(h[L_SAM]);
    np_fm = (int)h[L_PAIRS_FM].size() / 2; np_am = (int)h[L_PAIRS_AM].size() / 2; np_sam = (int)h[L_PAIRS_SAM].size() / 2;
    for (int i = 0; i < L_COUNT; i++) lists[i].n = (int)h[i].size();
    const std::vector<int> &fq = fq_lists.h[0];
    for (size_t i = 0; i < fq.size(); i += 2) { fq_lists.h[1].push_back(fq[i]); fq_lists.h[1].push_back(i + 1 < fq.size() ? fq[i + 1] : fq[i]); }
    np_fq = (int)fq_lists.h[1].size() / 2;
    ssql_lists.count(); fq_lists.count(); tap_lists.count(); gen_lists.count(); lms_long_lists.count();
}

// xsender / xsiphon (qh_taps.hpp): the lists at the first enable of either, the siphon's rings, indices and gains at its own (the sender's
// rows follow the call's length: process_chain)
int Engine::taps_alloc()
{
    if (!tap_lists.block) {
        if (int rc = quiesce()) return rc;
        if (int rc = list_make(tap_lists)) return rc;
    }
    if ((tap_lists[1].n || tap_lists[2].n) && !sip_ring) {
        if (int rc = quiesce()) return rc;
        if (int rc = alloc(sip_ring, (long long)nch * kSipSize, true)) return rc;       // create_siphon: malloc0, idx 0 (siphon.c:66-67)
        if (int rc = alloc(sip_idx, nch, true)) return rc;
        if (int rc = alloc(tap_gain, nch)) return rc;
        std::vector<double> g((size_t)nch);
        for (int ch = 0; ch < nch; ch++) {
            const ChanCfg &c = cfg[(size_t)ch];
            g[(size_t)ch] = (c.agc_run && c.agc_mode == 0 && !c.fix_before()) ? c.agc_fixed : 1.0;
        }
        QH_HIP(hipMemcpyAsync(tap_gain, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        QH_HIP(hipStreamSynchronize(stream));
    }
    return QH_OK;
}

// gen0 (qh_gen.hpp) at the first run of a channel's generator: state as create_gen leaves it (all zero: phases 0, the pulse OFF with
// pnoff samples to go, gen.c:86-87), every channel's parameters, the pulse's edge table
int Engine::gen_alloc()
{
    const double rate = (double)dsp_rate;
    if (int rc = quiesce()) return rc;
    if (int rc = list_make(gen_lists)) return rc;
    if (int rc = alloc(gen_prm, nch, true)) return rc;
    if (int rc = alloc(gen_state, nch, true)) return rc;
    if (int rc = alloc(gen_ck, (long long)nch * kGenCkMax, true)) return rc;
    // calc_pulse (gen.c:73-96) at create_gen's pf 0.25, duty 0.25, 2 ms edges: theta accumulates as there
    const double pperiod = 1.0 / 0.25;
    gen_pntrans = (int)(0.002 * rate);
    gen_pnon = (int)(0.25 * pperiod * rate);
    gen_pnoff = (int)(pperiod * rate) - gen_pnon - 2 * gen_pntrans;
    if (gen_pnoff < 0) gen_pnoff = 0;
    std::vector<double> ct((size_t)gen_pntrans + 1);
    const double delta = kPiRef / (double)gen_pntrans;
    double theta = 0.0;
    for (int i = 0; i <= gen_pntrans; i++) { ct[(size_t)i] = 0.5 * (1.0 - std::cos(theta)); theta += delta; }
    if (int rc = alloc(gen_ctrans, (long long)ct.size())) return rc;
    QH_HIP(hipMemcpyAsync(gen_ctrans, ct.data(), ct.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    if (carry.gen.size() == (size_t)nch)        // the state a new dsp_size left standing (Engine::rebuild)
        QH_HIP(hipMemcpyAsync(gen_state, carry.gen.data(), (size_t)nch * sizeof(GenState), hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));
    carry.gen.clear();
    gen_prm_h.assign((size_t)nch, GenParam{});
    for (ChanCfg &c : cfg) {
        c.w.gen_dirty = c.w.gen_sweep_dirty = true;
        c.w.gen_tone_reset = c.w.gen_sweep_reset = false;       // (the state is new)
    }
    return QH_OK;
}

// One channel's gen0 parameters.  The sweep's period and table come from the reference's own chain (sweep_walk), walked when a setter ran
// calc_sweep; setters that run calc_tone / calc_sweep also zero the phase (and the sweep's position) in stream order.
int Engine::prm_gen(ChanCfg &c, int ch)
{
    const double rate = (double)dsp_rate;
    GenParam &q = gen_prm_h[(size_t)ch];
    q.mode = c.gen_mode; q.pntrans = gen_pntrans; q.pnon = gen_pnon; q.pnoff = gen_pnoff;
    q.tone_mag = c.gen_tone_mag; q.tone_delta = kTwoPiRef * c.gen_tone_freq / rate;
    q.tt_mag1 = 0.5; q.tt_mag2 = 0.5; q.tt_delta1 = kTwoPiRef * 900.0 / rate; q.tt_delta2 = kTwoPiRef * 1700.0 / rate;      // gen.c:126-129
    q.noise_mag = c.gen_noise_mag;
    q.noise_key = gen_mix64((c.gen_seed_set ? c.gen_seed : kGenGolden * (unsigned long long)(ch + 1)) + kGenGolden * (unsigned long long)(ch + 1));
    q.sweep_mag = c.gen_sweep_mag;
    q.pulse_mag = 1.0; q.pulse_tdelta = kTwoPiRef * 1000.0 / rate;                                                         // gen.c:145-149
    if (c.w.gen_sweep_dirty) {
        const SweepWalk w = sweep_walk(rate, c.gen_sweep_f1, c.gen_sweep_f2, c.gen_sweep_rate, kGenWalkMax, kGenCkStep);
        q.sweep_P = w.P; q.sweep_dphs0 = w.dphs0; q.sweep_d2phs = w.d2phs; q.sweep_full = w.full;
        q.sweep_nck = (int)w.ck.size();
        if (q.sweep_nck > kGenCkMax) return set_error(QH_ERR_HIP, "gen0: sweep table of %d entries", q.sweep_nck);
        if (q.sweep_nck) {
            std::vector<double2> t(w.ck.size());
            for (size_t i = 0; i < t.size(); i++) t[i] = make_double2(w.ck[i].first, w.ck[i].second);
            QH_HIP(hipMemcpyAsync(gen_ck + (size_t)ch * kGenCkMax, t.data(), t.size() * sizeof(double2), hipMemcpyHostToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
        }
        c.w.gen_sweep_dirty = false;
    }
    if (c.w.gen_tone_reset) QH_HIP(hipMemsetAsync(&gen_state[ch].tone_phs, 0, sizeof(double), stream));                       // calc_tone, gen.c:31
    if (c.w.gen_sweep_reset) QH_HIP(hipMemsetAsync(&gen_state[ch].sweep_phs, 0, sizeof(double) + sizeof(long long), stream)); // calc_sweep, gen.c:51-52
    c.w.gen_tone_reset = c.w.gen_sweep_reset = false;
    QH_HIP(hipMemcpyAsync(gen_prm + ch, &q, sizeof(q), hipMemcpyHostToDevice, stream));
    c.w.gen_dirty = false;
    return QH_OK;
}

// what the setters changed since the last call, uploaded ahead of the call's launches
int Engine::refresh_gen()
{
    if (!gen_prm) return QH_OK;
    bool up = false;
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (!c.w.gen_dirty) continue;
        if (int rc = prm_gen(c, ch)) return rc;
        up = true;
    }
    if (up) QH_HIP(hipStreamSynchronize(stream));
    return QH_OK;
}

// The stages made when a channel first runs one of them (the lists' counts say which)
int Engine::stages_alloc()
{
    const double rate = (double)dsp_rate;
    if ((lists[L_AP].n || lists[L_AP + 1].n) && !ap_prm) if (int rc = ap_alloc()) return rc;
    if (ssql_lists.any() && !ssql_prm) if (int rc = ssql_alloc()) return rc;
    if (fq_lists[0].n && !fq_prm) if (int rc = fmsq_alloc()) return rc;
    if (tap_lists.any()) if (int rc = taps_alloc()) return rc;
    if (gen_lists[0].n && !gen_prm) if (int rc = gen_alloc()) return rc;
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
        for (ChanCfg &c : cfg) c.w.amsq_dirty = true;
    }
    bool any_lms = false;
    for (int k = 0; k < 6; k++) any_lms = any_lms || lms_n(k);
    if (any_lms && !lms_prm[0]) {
        for (int f = 0; f < 2; f++) {
            if (int rc = alloc(lms_prm[f], nch)) return rc;
            if (int rc = alloc(lms_state[f], nch)) return rc;
            // create_anf: lidx 1.0, ngamma 6.25e-12; create_anr: lidx 120.0, ngamma 0.001 (RXA.c:289-292,309-312)
            std::vector<LmsState> init((size_t)nch);
            std::memset(init.data(), 0, init.size() * sizeof(LmsState));
            for (LmsState &st : init) { st.lidx = f ? 120.0 : 1.0; st.ngamma = f ? 0.001 : 6.25e-12; }
            if (carry.lms[f].size() == 2 * (size_t)nch)         // what ran on across a new dsp_rate or dsp_size (Engine::rebuild)
                for (int ch = 0; ch < nch; ch++) { init[(size_t)ch].lidx = carry.lms[f][2 * (size_t)ch]; init[(size_t)ch].ngamma = carry.lms[f][2 * (size_t)ch + 1]; }
            carry.lms[f].clear();
            QH_HIP(hipMemcpyAsync(lms_state[f], init.data(), init.size() * sizeof(LmsState), hipMemcpyHostToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
        }
        for (ChanCfg &c : cfg) { c.w.lms[0].dirty = c.w.lms[1].dirty = true; c.w.lms[0].flush = c.w.lms[1].flush = false; }
    }
    // the long form's lists, and the rows of a filter that has a channel on them: zero, as create_anf / flush_anf leave w[] and d[]
    for (int f = 0; f < 2; f++) {
        if (!lms_long_lists[3 * f].n && !lms_long_lists[3 * f + 1].n && !lms_long_lists[3 * f + 2].n) continue;
        if (lms_long_lists.block && lms_long_rows[f]) continue;
        if (int rc = quiesce()) return rc;
        if (!lms_long_lists.block) if (int rc = list_make(lms_long_lists)) return rc;
        if (!lms_long_rows[f]) if (int rc = alloc(lms_long_rows[f], (long long)nch * kLmsLongRow, true)) return rc;
    }
    if (lists[L_LIM].n && !lim_prm) {
        if (int rc = alloc(lim_prm, nch)) return rc;
        if (int rc = alloc(lim_state, nch)) return rc;
        for (ChanCfg &c : cfg) c.w.lim_dirty = true;
    }
    return QH_OK;
}

// The channels that run stage f from here on.  A fircore keeps its delay lines while its channel is off the stage's list, and the
// ping-pong pair flips for the listed channels only: a channel that (re)joins the list finds its rows, short and long, in the half that
// was current when it left (Chan::at), and they move to the current one.  Called wherever the set of a stage's running channels may have
// changed, on either path; a stage that has not been made yet has nothing to follow.
int Engine::fc_follow(Fircore &f, const std::vector<int> &chans)
{
    if (!f.hist[0]) return QH_OK;
    for (Fircore::Chan &r : f.chan) { if (r.listed) r.at = f.cur; r.listed = false; }
    for (int ch : chans) {
        Fircore::Chan &r = f.chan[(size_t)ch];
        if (r.at != f.cur) {
            QH_HIP(hipMemcpyAsync(f.hist[f.cur] + (size_t)ch * kHistBand, f.hist[r.at] + (size_t)ch * kHistBand, (size_t)kHistBand * sizeof(double2),
                                  hipMemcpyDeviceToDevice, stream));
            if (f.lhist[0]) QH_HIP(hipMemcpyAsync(f.lhist[f.cur] + (size_t)ch * kLongHist, f.lhist[r.at] + (size_t)ch * kLongHist,
                                                  (size_t)kLongHist * sizeof(double2), hipMemcpyDeviceToDevice, stream));
        }
        r.at = f.cur;
        r.listed = true;
    }
    return QH_OK;
}

// setNc_fircore's flush (wdsp/firmin.c:454-466): zero n channels' delay lines of stage f from channel ch on, short and long, in both halves
int Engine::zero_rows(Fircore &f, int ch, int n)
{
    for (int i = 0; i < 2; i++) {
        QH_HIP(hipMemsetAsync(f.hist[i] + (size_t)ch * kHistBand, 0, (size_t)n * kHistBand * sizeof(double2), stream));
        if (f.lhist[i]) QH_HIP(hipMemsetAsync(f.lhist[i] + (size_t)ch * kLongHist, 0, (size_t)n * kLongHist * sizeof(double2), stream));
    }
    return QH_OK;
}

// Lists, stages and delay-line rows after a setter moved a channel between lists
int Engine::refresh_lists()
{
    std::vector<int> h[L_COUNT];
    build_lists(h);
    if (int rc = stages_alloc()) return rc;
    // bpsnba's fircore (the partitioned form's 16383-sample delay line goes along: nc > 4096)
    std::vector<int> snb(h[L_SNB]);
    snb.insert(snb.end(), h[L_SNB + 1].begin(), h[L_SNB + 1].end());
    if (int rc = fc_follow(fc[FC_SNB], snb)) return rc;
    // bp1's: SetRXABandpassRun (bandpass.c:385-390) switches it on without RXAbp1Set's flush (RXA.c:825)
    if (int rc = fc_follow(fc[FC_BP1], h[L_BP1])) return rc;
    // the FM de-emphasis / audio fircores' while the channel is in another mode (SetRXAMode only clears fmd's run flag, RXA.c:758-776)
    if (int rc = fc_follow(fc[FC_DE], h[L_FM])) return rc;
    if (int rc = fc_follow(fc[FC_AUD], h[L_FM])) return rc;
    // xfmsq's noise filter keeps its delay line while the stage is off (xfmsq with run 0 does not call its fircore, fmsq.c:143-147)
    if (int rc = fc_follow(fc[FC_FQ], fq_lists.h[0])) return rc;
    std::vector<int> all((size_t)nch * (L_COUNT + 3));
    for (int i = 0; i < L_COUNT; i++) std::copy(h[i].begin(), h[i].end(), all.begin() + (lists[i].dev - list_block));
    std::vector<double> fg((size_t)nch);
    for (int ch = 0; ch < nch; ch++) fg[(size_t)ch] = cfg[(size_t)ch].agc_fixed;
    QH_HIP(hipMemcpyAsync(list_block, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(fix_gain, fg.data(), fg.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    if (int rc = list_upload(ssql_lists)) return rc;
    if (int rc = list_upload(lms_long_lists)) return rc;
    if (int rc = list_upload(tap_lists)) return rc;
    if (int rc = list_upload(gen_lists)) return rc;
    if (int rc = list_upload(fq_lists)) return rc;
    QH_HIP(hipStreamSynchronize(stream));
    lists_dirty = false;
    fm_dirty = true;                // the design rows follow the running FM channels
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
    if (!c.w.agc_dirty) return QH_OK;
    // create_rxa's constants (RXA.c:335-358)
    const AgcParam q = load_wcpagc((double)dsp_rate, c.agc_tau_attack, c.agc_tau_decay, 4.0, c.agc_max_gain, c.agc_var_gain, c.agc_max_input, 1.0, 0.250, 0.005,
                                   5.0, 1, 0.500, c.agc_hangtime, c.agc_hang_thresh, 0.100);
    if (q.attack_buffsize + 2 > kAgcRing)
        return set_error(QH_ERR_UNSUPPORTED, "AGC attack of %g s needs a look-ahead of %d samples (limit %d)", c.agc_tau_attack,
                         q.attack_buffsize, kAgcRing - 2);
    c.w.agc_abuf = q.attack_buffsize;
    if (int rc = put_row(agc_prm, ch, q)) return rc;
    c.w.agc_dirty = false;
    return QH_OK;
}

int Engine::prm_emnr(ChanCfg &c, int ch)
{
    if (emnr_chan && c.w.emnr_dirty) {
        if (c.emnr_run && (c.emnr_npe < 0 || c.emnr_npe > 2 || c.emnr_gain_method < 0 || c.emnr_gain_method > 3))
            return set_error(QH_ERR_UNSUPPORTED, "EMNR: gain methods 0..3 and noise estimators 0..2");
        const EmnrChan ec{ c.emnr_gain_method, c.emnr_npe, c.emnr_ae, 0, c.emnr_ae_zeta, c.emnr_ae_psi, c.emnr_train_zeta, c.emnr_train_t2 };
        if (int rc = put_row(emnr_chan, ch, ec)) return rc;
        c.w.emnr_dirty = false;
    }
    if (emnr_state && c.w.emnr_flush) {           // flush_emnr, emnr.c:583-596: the accumulators and their indices, not the estimators
        EmnrScalars sc;
        QH_HIP(hipMemcpyAsync(&sc, emnr_scal + ch, sizeof(sc), hipMemcpyDeviceToHost, stream));
        QH_HIP(hipStreamSynchronize(stream));
        sc.iainidx = sc.iaoutidx = sc.oaoutidx = sc.nsamps = sc.saveidx = 0; sc.oainidx = emnr_prm.init_oainidx;
        if (int rc = put_row(emnr_scal, ch, sc, false)) return rc;
        QH_HIP(hipMemsetAsync(emnr_state + (size_t)ch * kEmnrStateDoubles, 0, (size_t)EO_PREVG * sizeof(double), stream));
        QH_HIP(hipStreamSynchronize(stream));
        c.w.emnr_flush = false;
    }
    return QH_OK;
}

int Engine::prm_snba(ChanCfg &c, int ch)
{
    const SnbaParam &q = snba_prm;
    if (snba_state && c.w.snba_taps_dirty) {
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
        c.w.snba_taps_dirty = false;
    }
    if (snba_state && (c.w.snba_flush || c.w.snba_rout_flush)) {
        double *st = snba_state + (size_t)ch * q.state_doubles;
        if (q.cpp_out > 1) QH_HIP(hipMemsetAsync(st + q.off_rout, 0, (size_t)(q.cpp_out - 1) * sizeof(double), stream));
        if (c.w.snba_flush) {         // flush_snba, snb.c:161-185: the frame half of xbase, the accumulators, both resamplers
            QH_HIP(hipMemsetAsync(st + kSnbX, 0, (size_t)kSnbX * sizeof(double), stream));
            QH_HIP(hipMemsetAsync(st + q.off_inacc, 0, (size_t)(q.state_doubles - q.off_inacc) * sizeof(double), stream));
            if (int rc = put_row(snba_idx, ch, SnbaIdx{ 0, 0, 0, 0, q.init_oaoutidx, { 0, 0, 0 } })) return rc;
        }
    }
    c.w.snba_flush = c.w.snba_rout_flush = false;
    return QH_OK;
}

int Engine::prm_amsq(ChanCfg &c, int ch)
{
    if (!amsq_prm || !c.w.amsq_dirty) return QH_OK;
    // calc_amsq, amsq.c:48-64: 10 ms average (RXA.c:165)
    const double rate = (double)dsp_rate;
    AmsqParam q{};
    q.avm = std::exp(-1.0 / (rate * 0.010)); q.onem_avm = 1.0 - q.avm;
    q.tail_thresh = c.amsq_tail_thresh; q.unmute_thresh = c.amsq_unmute_thresh; q.min_tail = 0.0; q.max_tail = c.amsq_max_tail;
    q.muted_gain = 0.0; q.rate = rate; q.ntup = amsq_ntup; q.ntdown = amsq_ntdown;
    if (int rc = put_row(amsq_prm, ch, q)) return rc;
    c.w.amsq_dirty = false;
    return QH_OK;
}

int Engine::prm_lms(ChanCfg &c, int ch)
{
    for (int f = 0; f < 2 && lms_prm[0]; f++) {
        const ChanCfg::Lms &m = c.lms[f];
        ChanCfg::Work::Lms &wm = c.w.lms[f];
        if (wm.dirty) {
            // lidx_min, lidx_max, den_mult, lincr, ldecr of create_rxa (RXA.c:290-295,310-315)
            if (int rc = put_row(lms_prm[f], ch, LmsParam{ m.taps, m.delay, f, 0, m.two_mu, m.gamma, f ? 120.0 : 0.0, 200.0, 6.25e-10, 1.0, 3.0 }))
                return rc;
            wm.dirty = false;
        }
        if (wm.flush) {          // flush_anf (anf.c:135-140): delay line and weights; lidx / ngamma carry on
            QH_HIP(hipMemsetAsync(lms_state[f] + ch, 0, offsetof(LmsState, lidx), stream));
            if (lms_long_rows[f]) QH_HIP(hipMemsetAsync(lms_long_rows[f] + (size_t)ch * kLmsLongRow, 0, (size_t)kLmsLongRow * sizeof(double), stream));
            wm.flush = false;
        }
    }
    return QH_OK;
}

int Engine::prm_lim(ChanCfg &c, int ch)
{
    if (!c.w.lim_dirty || !lim_prm) return QH_OK;
    // calc_fmd's create_wcpagc(1, 5, 1, ..., 0.001, 0.008, 4, lim_gain, 1.0, 1.0, 1.0, 0.9, 0.250, 0.004, 4.0, 0,
    // 0.500, 0.500, 2.000, 0.100) (fmd.c:48-72) through loadWcpAGC; a new limiter starts cleared
    const AgcParam q = load_wcpagc((double)dsp_rate, 0.001, 0.008, 4.0, c.lim_gain, 1.0, 1.0, 0.9, 0.250, 0.004, 4.0, 0, 0.500, 0.500, 2.000, 0.100);
    if (int rc = put_row(lim_prm, ch, q, false)) return rc;
    QH_HIP(hipMemsetAsync(lim_state + ch, 0, sizeof(AgcState), stream));
    if (int rc = put_row(&lim_state[ch].out_index, 0, kAgcRing - 1)) return rc;        // out_index = -1 (calc_wcpagc, wcpAGC.c:34)
    c.w.lim_dirty = false;
    return QH_OK;
}

// the detectors' own parameters: AM's fade leveller, SAM's sideband mode, FM's gain and its CTCSS notch
int Engine::prm_detect(ChanCfg &c, int ch)
{
    if (!c.w.demod_dirty) return QH_OK;
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
    if (c.w.ctcss_flush) {                    // calc_snotch ends with flush_snotch, wdsp/iir.c:48
        QH_HIP(hipMemsetAsync(sn_state + ch, 0, sizeof(SnotchState), stream));
        c.w.ctcss_flush = false;
    }
    QH_HIP(hipStreamSynchronize(stream));
    c.w.demod_dirty = false;
    return QH_OK;
}

// Room for `rows` design rows of an FM filter's masks (and of its partitions' masks where the stage has them): one row is the shared row
// (stride 0, no mask_row), more are rows of kBandNfftMax with the channels' row numbers beside them.  What the rows held is lost.
int Engine::fm_rows_resize(Fircore &f, int rows)
{
    if (int rc = quiesce()) return rc;
    f.rows = rows;
    f.mask_stride = rows > 1 ? kBandNfftMax : 0;
    if (int rc = alloc(f.mask, (long long)rows * kBandNfftMax)) return rc;
    if (rows > 1) { if (int rc = alloc(f.mask_row, nch, true)) return rc; }
    else release(f.mask_row);
    if (f.lmask) {
        if (int rc = alloc(f.lmask, (long long)rows * kLongParts * kBandNfftMax, true)) return rc;
        if (int rc = alloc(f.lrow_parts, rows, true)) return rc;
    }
    return QH_OK;
}

// create_fmd, wdsp/fmd.c:108-118: every channel's de-emphasis (pde) and audio (paud) filter, one mask row per distinct design among the
// running FM channels -- (nc, mp, f_low, f_high) of the filter; dsp_rate, dsp_size and the masks' layout are the engine's.  Rows are
// numbered in the order the channels first ask for them.  A row whose design stood on the device before is not designed again (its taps
// are kept: it is uploaded again only where it moved or the masks were laid out anew); SetRXAFMNCde / NCaud's flush of the one line.
int Engine::fm_filters()
{
    if (fm_key_built != mask_key()) fm_dirty = fm_relayout = true;
    if (!fm_dirty) return QH_OK;
    const double rate = (double)dsp_rate, afgain = 0.5;
    for (int s = 0; s < 2; s++) {
        Fircore &f = fc[s ? FC_AUD : FC_DE];
        std::vector<FmRow> want;
        std::vector<int> row_of((size_t)nch, 0);
        for (int ch = 0; ch < nch; ch++) {
            ChanCfg &c = cfg[(size_t)ch];
            bool &flush = s ? c.w.fm_aud_flush : c.w.fm_de_flush;
            if (flush) { if (int rc = zero_rows(f, ch)) return rc; flush = false; }      // setNc_fircore, firmin.c:455-467
            if (!c.fmd_run) continue;
            FmRow k;
            k.nc = s ? c.fm_nc_aud : c.fm_nc_de; k.mp = s ? c.fm_mp_aud : c.fm_mp_de; k.f_low = c.fm_f_low; k.f_high = c.fm_f_high;
            size_t r = 0;
            while (r < want.size() && !want[r].same(k)) r++;
            if (r == want.size()) want.push_back(k);
            row_of[(size_t)ch] = (int)r;
        }
        if (want.empty()) continue;
        std::vector<FmRow> &built = fm_rows[s];
        const bool resized = (int)want.size() != f.rows;
        if (resized) if (int rc = fm_rows_resize(f, (int)want.size())) return rc;
        std::vector<char> fresh(want.size(), 0);
        for (size_t r = 0; r < want.size(); r++) {
            FmRow &w = want[r];
            fresh[r] = resized || fm_relayout || r >= built.size() || !built[r].same(w);
            for (FmRow &b : built) if (b.same(w) && !b.taps.empty()) { w.taps = b.taps; w.real = b.real; break; }
            if (!w.taps.empty()) continue;
            // de-emphasis by frequency sampling (fmd.c:112), audio band-pass 0.8 f_low .. 1.1 f_high (fmd.c:115)
            w.taps = s ? fir_bandpass(w.nc, 0.8 * w.f_low, 1.1 * w.f_high, rate, 0, 1, afgain / (2.0 * dsp_size))
                       : fc_impulse(w.nc, w.f_low, w.f_high, +20.0 * std::log10(w.f_high / w.f_low), 0.0, 1, rate, 1.0 / (2.0 * dsp_size), 0, 0);
            if (w.mp) w.taps = mp_imp(w.taps, 16, 0);           // SetRXAFMMPde / MPaud, fmd.c:295-305,324-334
            for (cd &v : w.taps) v *= (double)(2 * dsp_size);
            w.real = true;
            for (const cd &v : w.taps) w.real = w.real && v.imag() == 0.0;
            fm_designed++;
        }
        for (size_t r = 0; r < want.size(); r++) {
            if (!fresh[r]) continue;
            std::vector<cd> m;
            if (int rc = put_taps(f, (int)r, want[r].taps, m)) return rc;
        }
        if (f.mask_row && (resized || row_of != fm_row_of[s])) {
            QH_HIP(hipMemcpyAsync(f.mask_row, row_of.data(), (size_t)nch * sizeof(int), hipMemcpyHostToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
        }
        built = std::move(want);
        fm_row_of[s] = std::move(row_of);
    }
    // a row with a complex tap (minimum phase) takes no partner: the paired tile is for real filters, so the stage then runs unpaired
    de_real = true;
    for (const FmRow &r : fm_rows[0]) de_real = de_real && r.real;
    fm_key_built = mask_key();
    fm_dirty = fm_relayout = false;
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
        if (!c.w.agc_dirty || !c.w.agc_ran) continue;
        const int abuf = (int)std::ceil((double)dsp_rate * 4.0 * c.agc_tau_attack);
        if (c.w.agc_abuf != abuf) { c.w.agc_rewindow = true; if (!c.w.agc_stale) { c.w.agc_stale = true; lists_dirty = true; } }
    }
    if (lists_dirty) if (int rc = refresh_lists()) return rc;
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (int rc = prm_agc(c, ch)) return rc;
        if (int rc = prm_emnr(c, ch)) return rc;
        if (int rc = prm_snba(c, ch)) return rc;
        if (int rc = prm_amsq(c, ch)) return rc;
        if (int rc = prm_fmsq(c, ch)) return rc;
        if (int rc = prm_lms(c, ch)) return rc;
        if (int rc = prm_lim(c, ch)) return rc;
        if (int rc = prm_detect(c, ch)) return rc;
    }
    if (int rc = fm_filters()) return rc;
    return fmsq_filter();
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
    wide.snba_ovrlp = ovrlp;
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

// What calc_snba's integer divisions (snb.c:33-36) leave consistent: a whole ratio to the 12 kHz internal rate that the kernels are made
// for (1 .. kSnbMaxRatio, powers of two) and a block the ratio divides, so that isize * ratio is dsp_size.
bool Engine::snba_accepts(int rate, int size)
{
    if (rate < 12000 || rate % 12000) return false;
    const int ratio = rate / 12000;
    return ratio <= kSnbMaxRatio && (ratio & (ratio - 1)) == 0 && size > 0 && size <= kSnbMaxDsp && size % ratio == 0;
}

// calc_snba (wdsp/snb.c:31-66) with create_rxa's arguments (RXA.c:237-255): parameters, both resamplers' taps, the state of every channel
int Engine::snba_alloc()
{
    // calc_snba, snb.c:31-66, with create_rxa's arguments (RXA.c:237-255)
    SnbaParam &q = snba_prm;
    if (!snba_accepts(dsp_rate, dsp_size)) return set_error(QH_ERR_UNSUPPORTED, "%s", snba_accepted());
    q.ratio = dsp_rate / 12000;
    q.isize = dsp_size / q.ratio;
    q.cpp_in = q.ratio > 1 ? 140 * q.ratio + 1 : 1;
    q.cpp_out = q.ratio > 1 ? 141 : 1;
    q.asize = 64; q.npasses = 2; q.b = 10; q.pre = 2; q.post = 2; q.k1 = 8.0; q.k2 = 20.0; q.pmultmin = 0.5;
    snba_plan(wide.snba_ovrlp);
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
    if (carry.snba_frames.size() == (size_t)nch * 2 * kSnbX)    // the frame memory stays across decalc_snba / calc_snba (Engine::rebuild)
        QH_HIP(hipMemcpy2DAsync(snba_state, (size_t)q.state_doubles * sizeof(double), carry.snba_frames.data(), 2 * kSnbX * sizeof(double),
                                2 * kSnbX * sizeof(double), (size_t)nch, hipMemcpyHostToDevice, stream));
    if (int rc = fc_alloc(fc[FC_SNB])) return rc;
    QH_HIP(hipStreamSynchronize(stream));
    carry.snba_frames.clear();
    for (ChanCfg &c : cfg) { c.w.snba_taps_dirty = true; c.w.snb_dirty = true; c.w.snba_flush = c.w.snba_rout_flush = false; c.w.snb_flush = false; }
    return QH_OK;
}

// calc_emnr (wdsp/emnr.c:240-497) with create_rxa's arguments (RXA.c:319-332): parameters, window, start values of every array
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
    q.z_gamma_min = wide.h_zrange[0]; q.z_gamma_max = wide.h_zrange[1]; q.z_xihat_min = wide.h_zrange[2]; q.z_xihat_max = wide.h_zrange[3];
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
    QH_HIP(hipMemcpyAsync(emnr_GG, wide.h_GG.data(), wide.h_GG.size() * 8, hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(emnr_GGS, wide.h_GGS.data(), wide.h_GGS.size() * 8, hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(emnr_zeta, wide.h_zeta.data(), wide.h_zeta.size() * 8, hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(emnr_zeta_true, wide.h_zeta_true.data(), wide.h_zeta_true.size() * 4, hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));
    if (int rc = emnr_lds_limit()) return rc;
    for (ChanCfg &c : cfg) { c.w.emnr_dirty = true; c.w.emnr_flush = false; }
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

// partials of the fused meters: one per tile and row of 16 lanes
int Engine::ensure_meter_partials(long long n_mid, int lout)
{
    const long long need = ((n_mid + lout - 1) / lout) * meter_parts();
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

int Engine::long_stage_alloc(Fircore &f)
{
    if (f.lmask) return QH_OK;
    if (int rc = quiesce()) return rc;
    const long long rows = f.mask_rows(nch);
    if (int rc = alloc(f.lmask, rows * kLongParts * kBandNfftMax, true)) return rc;
    if (int rc = alloc(f.lrow_parts, rows, true)) return rc;
    for (double2 *&h : f.lhist) if (int rc = alloc(h, (long long)nch * kLongHist, true)) return rc;
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
int Engine::long_masks_upload(Fircore &f, long long row, const std::vector<cd> &h)
{
    std::vector<cd> all((size_t)kLongParts * kBandNfftMax, cd(0.0, 0.0));
    const int own = (int)std::min<size_t>((h.size() + kLongPart - 1) / kLongPart, (size_t)kLongParts);
    for (int p = 0; p < own; p++) {
        const size_t a = (size_t)p * kLongPart, b = std::min(h.size(), a + (size_t)kLongPart);
        const std::vector<cd> m = make_mask(std::vector<cd>(h.begin() + (long)a, h.begin() + (long)b), kBandNfftMax);
        std::copy(m.begin(), m.end(), all.begin() + (long)((size_t)p * kBandNfftMax));
    }
    QH_HIP(hipMemcpyAsync(f.lmask + (size_t)row * kLongParts * kBandNfftMax, all.data(), all.size() * sizeof(cd), hipMemcpyHostToDevice, stream));
    return put_row(f.lrow_parts, row, own);
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

// The tile length of a stage that runs one lane per tile (audio peak, SSQL) over `rows` listed channels: tiles short enough for about
// four wavefronts of 64 tiles per SIMD (1024 SIMDs), 256 .. 8192 samples
static int lane_tile_len(int rows, long long n_mid)
{
    int L = 256;
    while (L < 8192 && (long long)rows * n_mid / L > 4LL * 64 * 1024) L *= 2;
    return L;
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
    for (ChanCfg &c : cfg) { c.w.ap_dirty = true; c.w.sp_flush = false; for (bool &f : c.w.mp_flush) f = false; }    // the state starts at zero
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
        for (ChanCfg &c : cfg) { c.w.sp_flush = false; for (bool &f : c.w.mp_flush) f = false; }
        return QH_OK;
    }
    const int nap = k.mixed ? lists[L_AP].n + lists[L_AP + 1].n : 0;
    int L = ap_L;
    if (nap) {
        L = lane_tile_len(nap, k.n_mid);
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
        if (c.w.sp_flush || c.w.mp_flush[0] || c.w.mp_flush[1]) {            // flush_speak: that cascade's x / y history, I and Q
            for (int comp = 0; comp < 2; comp++) {
                double *st = ap_state + (size_t)ch * kApW + (size_t)comp * kApDim;
                if (c.w.sp_flush) QH_HIP(hipMemsetAsync(st + kApSpeakAt, 0, kApCascade * sizeof(double), stream));
                for (int p = 0; p < kApPeaks; p++)
                    if (c.w.mp_flush[p]) QH_HIP(hipMemsetAsync(st + kApPeakAt + kApCascade * p, 0, kApCascade * sizeof(double), stream));
            }
            c.w.sp_flush = false;
            for (bool &f : c.w.mp_flush) f = false;
        }
        if (!c.w.ap_dirty && !(nap && L != ap_L && c.ap_on())) continue;
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
        c.w.ap_dirty = false;
        up = true;
    }
    if (up) QH_HIP(hipStreamSynchronize(stream));
    ap_L = L;
    return QH_OK;
}

// ---- xssql (qh_ssql.hpp)
int Engine::ssql_alloc()
{
    const double rate = (double)dsp_rate;
    if (int rc = list_make(ssql_lists)) return rc;
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
    for (ChanCfg &c : cfg) c.w.ssql_dirty = true;
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
        L = lane_tile_len(nss, k.n_mid);       // (a multiple of 64: whole words)
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
        if (!c.w.ssql_dirty && !(nss && L != ssql_L && c.ssql_on())) continue;
        SsqlParam &q = ssql_prm_h[(size_t)ch];
        q = base;
        q.wthresh = c.ssql_wthresh;
        q.mute_mult = 1.0 - std::exp(-1.0 / (rate * c.ssql_tau_mute));            // ssql.c:137-138, :339-370
        q.unmute_mult = 1.0 - std::exp(-1.0 / (rate * c.ssql_tau_unmute));
        QH_HIP(hipMemcpyAsync(ssql_prm + ch, &q, sizeof(q), hipMemcpyHostToDevice, stream));
        c.w.ssql_dirty = false;
        up = true;
    }
    if (up) QH_HIP(hipStreamSynchronize(stream));
    if (nss) ssql_L = L;
    return QH_OK;
}

// ---- xfmsq (qh_fmsq.hpp)
int Engine::fmsq_alloc()
{
    const double rate = (double)dsp_rate;
    if (int rc = list_make(fq_lists)) return rc;
    if (int rc = alloc(fq_prm, nch)) return rc;
    if (int rc = alloc(fq_state, nch)) return rc;
    if (int rc = fc_alloc(fc[FC_FQ])) return rc;
    // the ready delay (fmsq.c:153-154, tdelay 0.100: RXA.c:224): the additions of rstep that take ramp to tdelay, counted as they are made
    {
        const double rstep = 1.0 / rate, tdelay = 0.100;
        double ramp = 0.0;
        fq_nready = 0;
        do { ramp += rstep; fq_nready++; } while (!(ramp >= tdelay));
    }
    // calc_fmsq (fmsq.c:50-78): avnoise 100, longnoise 1, MUTED, not ready; tup 0.050, tdown 0.010 (RXA.c:227-228), theta accumulates as there
    FmsqState z{};
    z.avnoise = 100.0; z.longnoise = 1.0; z.state = FQ_MUTED; z.count = 0; z.wait = fq_nready;
    std::vector<FmsqState> st((size_t)nch, z);
    QH_HIP(hipMemcpyAsync(fq_state, st.data(), st.size() * sizeof(FmsqState), hipMemcpyHostToDevice, stream));
    fq_ntup = (int)(0.050 * rate); fq_ntdown = (int)(0.010 * rate);
    std::vector<double> up((size_t)fq_ntup + 1), down((size_t)fq_ntdown + 1);
    double delta = kPiRef / (double)fq_ntup, theta = 0.0;
    for (int i = 0; i <= fq_ntup; i++) { up[(size_t)i] = 0.5 * (1.0 - std::cos(theta)); theta += delta; }
    delta = kPiRef / (double)fq_ntdown; theta = 0.0;
    for (int i = 0; i <= fq_ntdown; i++) { down[(size_t)i] = 0.5 * (1 + std::cos(theta)); theta += delta; }
    if (int rc = alloc(fq_cup, (long long)up.size())) return rc;
    if (int rc = alloc(fq_cdown, (long long)down.size())) return rc;
    QH_HIP(hipMemcpyAsync(fq_cup, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    QH_HIP(hipMemcpyAsync(fq_cdown, down.data(), down.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    QH_HIP(hipStreamSynchronize(stream));
    fq_nc_built = 0;
    for (ChanCfg &c : cfg) c.w.fmsq_dirty = true;
    return QH_OK;
}

int Engine::prm_fmsq(ChanCfg &c, int ch)
{
    if (!fq_prm || !c.w.fmsq_dirty) return QH_OK;
    // calc_fmsq, fmsq.c:48-53 with avtau 0.001, longtau 0.100, min_tail 0, max_tail 1.2 (RXA.c:225-226,231-232)
    const double rate = (double)dsp_rate;
    FmsqParam q{};
    q.avm = std::exp(-1.0 / (rate * 0.001)); q.onem_avm = 1.0 - q.avm;
    q.longavm = std::exp(-1.0 / (rate * 0.100)); q.onem_longavm = 1.0 - q.longavm;
    q.tail_thresh = c.fmsq_tail_thresh; q.unmute_thresh = c.fmsq_unmute_thresh; q.min_tail = 0.000; q.max_tail = 1.200;
    q.rate = rate; q.ntup = fq_ntup; q.ntdown = fq_ntdown;
    if (int rc = put_row(fq_prm, ch, q)) return rc;
    c.w.fmsq_dirty = false;
    return QH_OK;
}

// The noise filter the engine's FMSQ channels share (calc_fmsq, fmsq.c:36-46; SetRXAFMSQNC / MP, fmsq.c:252-279), rebuilt when their
// nc, mp or the band tile moved.  A minimum-phase design keeps the real parts of mp_imp's taps, so that the stage stays a real filter (two
// channels a tile): the response of a real even filter has a real minimum-phase form, and what the cepstral method leaves beside it on
// its 16 nc-point grid is 4e-10 of the largest tap at nc 4096.  With taps yr + j yi on the signal (t, t) the reference's noise is
// sqrt(2 (yr^2 + yi^2)): the residue enters in second order (tests/test_design_eq_host.py holds it under 1e-12 of the noise's RMS).
int Engine::fmsq_filter()
{
    if (!fq_prm || !fq_lists[0].n) return QH_OK;
    const ChanCfg &c = cfg[(size_t)fq_lists.h[0][0]];        // (chain_needs has refused FMSQ channels that differ)
    if (c.fmsq_nc == fq_nc_built && c.fmsq_mp == fq_mp_built && fq_key_built == mask_key()) return QH_OK;
    std::vector<cd> h = fmsq_impulse(c.fmsq_nc, (double)dsp_rate, 1.0 / (2.0 * dsp_size));
    if (c.fmsq_mp) h = mp_imp(h, 16, 0);
    for (auto &v : h) v = cd(v.real() * (double)(2 * dsp_size), 0.0);
    std::vector<cd> m;
    if (int rc = put_taps(fc[FC_FQ], 0, h, m)) return rc;
    if (fq_nc_built && fq_nc_built != c.fmsq_nc) if (int rc = zero_rows(fc[FC_FQ], 0, nch)) return rc;       // setNc_fircore zeroes the delay line
    fq_nc_built = c.fmsq_nc; fq_mp_built = c.fmsq_mp; fq_key_built = mask_key();
    return QH_OK;
}

// ---- xeqp (wdsp/eq.c:166-208)
// The taps a channel's fircore holds: eq_impulse as create_eqp and the setters call it (eq.c:185), through mp_imp when mp is set
// (calc_fircore, firmin.c:327-328), its complex taps kept as fircore uses them.  Scale 1 / (2 dsp_size), as there.
std::vector<cd> Engine::eqp_taps(const ChanCfg &c) const
{
    std::vector<cd> h = eq_impulse(c.eqp_nc, (int)c.eqp_F.size() - 1, c.eqp_F.data(), c.eqp_G.data(), (double)dsp_rate, 1.0 / (2.0 * dsp_size), c.eqp_ctfmode,
                                   c.eqp_wintype);
    if (c.eqp_mp) h = mp_imp(h, 16, 0);
    return h;
}

int Engine::eqp_alloc()
{
    if (int rc = quiesce()) return rc;
    if (int rc = list_make(eq_lists)) return rc;
    if (int rc = fc_alloc(fc[FC_EQP])) return rc;
    for (ChanCfg &c : cfg) { c.w.eqp_dirty = true; c.w.eqp_flush = false; }
    return QH_OK;
}

// The equalizer's channel lists, delay-line rows and masks after a setter, a change of the band tile or of the two-group layout.
// SetRXAEQNC with a new nc zeroes the channel's delay line (setNc_fircore); every other setter swaps the mask and keeps the line
// (setImpulse_fircore(..., 1)); a channel that does not run the stage keeps its line where it was (xeqp, eq.c:204-207).
int Engine::refresh_eqp()
{
    Fircore &eq = fc[FC_EQP];
    if (eq_lists_dirty) {
        eq_lists.clear();
        for (int ch = 0; ch < nch; ch++) eq_lists.h[cfg[(size_t)ch].eqp_run ? 0 : 1].push_back(ch);
        if (!eq_lists.h[0].empty() && !eq.mask) if (int rc = eqp_alloc()) return rc;
        eq_lists.count();
        if (!eq.mask) eq_lists.row[1].n = 0;
        if (eq.mask) {
            if (int rc = fc_follow(eq, eq_lists.h[0])) return rc;
            if (int rc = list_upload(eq_lists)) return rc;
            QH_HIP(hipStreamSynchronize(stream));
        }
        eq_lists_dirty = false;
    }
    if (!eq.mask) return QH_OK;
    if (eq_key_built != mask_key()) { for (ChanCfg &c : cfg) c.w.eqp_dirty = true; eq_key_built = mask_key(); }
    std::vector<cd> last_h, last, last_taps;
    const ChanCfg *last_cfg = nullptr;
    if (eq_taps_h.size() != (size_t)nch) eq_taps_h.assign((size_t)nch, std::vector<cd>());
    for (int ch = 0; ch < nch; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (c.w.eqp_flush) {
            if (int rc = zero_rows(eq, ch)) return rc;
            c.w.eqp_flush = false;
        }
        if (!c.eqp_run || !c.w.eqp_dirty) continue;       // (a channel that does not run keeps eqp_dirty until it does)
        const bool same = last_cfg && last_cfg->eqp_nc == c.eqp_nc && last_cfg->eqp_mp == c.eqp_mp && last_cfg->eqp_ctfmode == c.eqp_ctfmode &&
                          last_cfg->eqp_wintype == c.eqp_wintype && last_cfg->eqp_F == c.eqp_F && last_cfg->eqp_G == c.eqp_G;
        if (!same) {
            last_h = last_taps = eqp_taps(c);
            for (auto &v : last_h) v *= (double)(2 * dsp_size);      // the engine's mask convention, as fmsq_filter
            last.clear();
            last_cfg = &c;
        }
        if (int rc = put_taps(eq, ch, last_h, last)) return rc;
        eq_taps_h[(size_t)ch] = last_taps;
        c.w.eqp_dirty = false;
    }
    return QH_OK;
}

// flush_rxa (wdsp/RXA.c:527-559): NCO phase, resampler ring and fircore delay lines back to zero
int Engine::flush()
{
    epoch++;
    QH_HIP(hipSetDevice(device));
    QH_HIP(hipMemsetAsync(nco_phase, 0, (size_t)nch * sizeof(unsigned long long), stream));
    QH_HIP(hipMemsetAsync(nco_parked, 0, (size_t)nch * sizeof(unsigned long long), stream));
    if (rsmpout) if (int rc = qh_rat_reset(rsmpout)) return rc;        // flush_resample, wdsp/resample.c:159-165
    if (rsmpin) if (int rc = qh_rat_reset(rsmpin)) return rc;
    for (int i = 0; i < 2; i++) {
        if (hist_front[i]) QH_HIP(hipMemsetAsync(hist_front[i], 0, (size_t)nch * kHistFront * sizeof(double2), stream));
    }
    // the fircore stages that have been made: flush_nbp, flush_bandpass, flush_fmd, flush_bpsnba, flush_fmsq, flush_eqp (RXA.c:536-549).
    // (bpsnba's short rows were left to snb_flush and the next refresh_params; that zeroes them on this stream ahead of the next call's
    // launches, which nothing on the stream can tell from zeroing them here.)
    for (Fircore &f : fc) if (f.hist[0]) if (int rc = zero_rows(f, 0, nch)) return rc;
    if (demod_alloc) {                        // flush_wcpagc zeroes the ring (wcpAGC.c:154-159)
        for (int c = 0; c < nch; c++) {
            QH_HIP(hipMemsetAsync(agc_state[c].ring, 0, sizeof(agc_state[c].ring), stream));
            QH_HIP(hipMemsetAsync(agc_state[c].abs_ring, 0, sizeof(agc_state[c].abs_ring), stream));
            QH_HIP(hipMemsetAsync(&agc_state[c].ring_max, 0, sizeof(double), stream));
            if (cfg[(size_t)c].w.agc_stale) lists_dirty = true;
            cfg[(size_t)c].w.agc_stale = false;     // an empty ring and ring_max = 0: nothing stale (qh_agc_tiled.hpp)
        }
        if (agc_lring) {
            QH_HIP(hipMemsetAsync(agc_lring, 0, (size_t)nch * kAgcLongRing * sizeof(double2), stream));
            QH_HIP(hipMemsetAsync(agc_labs, 0, (size_t)nch * kAgcLongRing * sizeof(double), stream));
        }
    }
    for (ChanCfg &c : cfg) { c.w.lms[0].flush = c.w.lms[1].flush = true; c.w.emnr_flush = true; c.w.snba_flush = true; }    // flush_anf / flush_anr / flush_emnr, RXA.c:541-543
    if (amsq_state) QH_HIP(hipMemsetAsync(amsq_state, 0, (size_t)nch * sizeof(AmsqState), stream));     // flush_amsq
    if (ap_state) QH_HIP(hipMemsetAsync(ap_state, 0, (size_t)nch * kApW * sizeof(double), stream));    // flush_cbl / _speak / _mpeak, RXA.c:553-555
    if (ssql_state) launch_ssql_flush();        // flush_ssql, RXA.c:556
    if (snd_rows) QH_HIP(hipMemsetAsync(snd_rows, 0, (size_t)nch * (size_t)snd_cap * sizeof(float2), stream));       // flush_sender, RXA.c:538
    if (sip_ring) {                             // flush_siphon, RXA.c:552 (siphon.c:88-94)
        QH_HIP(hipMemsetAsync(sip_ring, 0, (size_t)nch * kSipSize * sizeof(double2), stream));
        QH_HIP(hipMemsetAsync(sip_idx, 0, (size_t)nch * sizeof(int), stream));
    }
    if (gen_state)                              // flush_gen, RXA.c:534 (gen.c:160-163): the pulse's state machine alone
        hipLaunchKernelGGL(gen_flush_kernel, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, stream, nch, (const GenParam *)gen_prm, gen_state);
    if (fq_state) launch_fmsq_flush();          // flush_fmsq, RXA.c:544 (its noise filter's lines: above)
    if (demod_alloc) {                        // flush_amd / flush_fmd / flush_snotch
        QH_HIP(hipMemsetAsync(am_state, 0, (size_t)nch * sizeof(AmState), stream));
        QH_HIP(hipMemsetAsync(pll_state, 0, (size_t)nch * sizeof(PllState), stream));
        QH_HIP(hipMemsetAsync(fm_pll_state, 0, (size_t)nch * sizeof(PllState), stream));
        QH_HIP(hipMemsetAsync(sn_state, 0, (size_t)nch * sizeof(SnotchState), stream));
    }
    return QH_OK;
}

// ---- the run-time setters of wdsp/channel.c:169-258 on a live engine ---------------------------------------------------------
// SetInputSamplerate, SetOutputSamplerate, SetDSPSamplerate, SetDSPBuffsize and SetAllRates as one call: any subset of the four values
// may differ from the current ones.  What the reference does to each stage (setInputSamplerate_rxa ... setDSPBuffsize_rxa, RXA.c:600-740,
// and every stage's setSamplerate_* / setSize_*) is tabled in DESIGN.md row b24; in short:
//   in_rate   shift restarts at phase 0 (shift.c:93-98), rsmpin is made anew (resample.c:171-176), nothing at the DSP rate is touched
//   out_rate  rsmpout is made anew (resample.c:178-183), nothing else is touched
//   dsp_rate  every stage at the DSP rate is designed again from the kept settings; both resamplers and most state start from zero
//             (decalc / calc or flush).  Kept: the delay lines of nbp0, bp1, eqp and xfmd's two filters (a new impulse response only),
//             anf / anr's lidx and ngamma, snba's frame memory, the SAM detector's sideband all-pass chains
//   dsp_size  the same without the redesign, but setSize_fircore re-plans those five filters, so their delay lines go; setSize_amd keeps
//             the whole AM / SAM detector and setSize_gen all of gen0 but the pulse's state
// The first two are done in place: only the front stage or rsmpout is made again, every other buffer and all state run on.  The last two
// leave so little standing that the engine is made anew in place (rebuild) with the settings and the kept state carried over.
// A refused call returns the status qh_rxa_create would set and has changed nothing.
int Engine::set_rates(int new_in, int new_dsp, int new_out, int new_size)
{
    if (new_in == in_rate && new_dsp == dsp_rate && new_out == out_rate && new_size == dsp_size) return QH_OK;
    int new_D = 0;
    if (int rc = check_rates("qh_rxa_set_rates", new_size, new_in, new_dsp, new_out, &new_D)) return rc;
    for (const ChanCfg &c : cfg) {
        // setSize_nbp / setSize_bandpass: "'size' must be <= 'nc'" (nbp.c:308, bandpass.c:345); the other fircores are planned the same way
        const int nc = std::min({ c.nbp_nc, c.snb_nc, c.bp1_nc, c.fm_nc_de, c.fm_nc_aud, c.fmsq_nc, c.eqp_nc });
        if (new_size > nc) return set_error(QH_ERR_UNSUPPORTED, "dsp_size %d above nc %d of channel %d: size must be <= nc (wdsp/nbp.c:308)", new_size, nc, (int)(&c - cfg.data()));
        if (c.emnr_run && new_size > kEmnrIncr) return set_error(QH_ERR_UNSUPPORTED, "EMNR: dsp_size up to %d", kEmnrIncr);
        if (c.snba_run && !snba_accepts(new_dsp, new_size)) return set_error(QH_ERR_UNSUPPORTED, "%s", snba_accepted());
    }
    if (wide.disp && qh_ana_buff_size(wide.disp) != new_size)
        return set_error(QH_ERR_INVALID, "the attached display bank has buff_size %d: detach it before dsp_size becomes %d", qh_ana_buff_size(wide.disp), new_size);
    QH_HIP(hipSetDevice(device));
    if (new_dsp != dsp_rate || new_size != dsp_size) return rebuild(new_in, new_dsp, new_out, new_size, new_D);
    if (int rc = quiesce()) return rc;
    if (new_in != in_rate) {        // setInputSamplerate_rxa, RXA.c:600-614
        in_rate = new_in; D = new_D;
        if (int rc = front_build()) return rc;
        if (int rc = tile_lds_limits()) return rc;
        QH_HIP(hipMemsetAsync(nco_phase, 0, (size_t)nch * sizeof(unsigned long long), stream));         // setSamplerate_shift, shift.c:93-98
        QH_HIP(hipMemsetAsync(nco_parked, 0, (size_t)nch * sizeof(unsigned long long), stream));
        for (ChanCfg &c : cfg) c.w.nco_dirty = true;          // calc_shift: delta is per sample of the new rate
    }
    if (new_out != out_rate) {      // setOutputSamplerate_rxa, RXA.c:616-625
        out_rate = new_out;
        if (int rc = out_build()) return rc;
    }
    QH_HIP(hipStreamSynchronize(stream));
    return QH_OK;
}

// A channel's settings as a setter list replayed on a fresh engine would leave them: every value kept, every note of work pending or
// done (ChanCfg::Work) as ChanCfg() has it.
static ChanCfg settings_of(const ChanCfg &o, int dsp_rate)
{
    ChanCfg c = o;
    c.w = ChanCfg::Work();
    c.snba_f_low = ChanCfg().snba_f_low; c.snba_f_high = ChanCfg().snba_f_high;     // calc_snba makes outresamp with its creation arguments (snb.c:43-44)
    c.w.eqp_tie = eqp_profile_tie(c.eqp_F, c.eqp_G, (double)dsp_rate);
    return c;
}

// A new dsp_rate or dsp_size (setDSPSamplerate_rxa, setDSPBuffsize_rxa: RXA.c:627-740).  The engine is destroyed and constructed again
// where it stands -- same handle, lock, stream, device and channel count -- so every buffer goes through alloc() and `owned` again and
// every stage starts as create_rxa leaves it.  Carried over: the channels' settings (settings_of: all of ChanCfg but its Work) and the
// engine-wide ones (Engine::Wide), and of the state
//   dsp_rate alone   the delay lines of nbp0, bp1, eqp and xfmd's two filters, where the stage holds its one-tile form (nc <= 4096; a
//                    partitioned stage's 65535-sample line is not carried and starts from zero: a stated deviation);
//                    the SAM detector's sideband chains (init_amd leaves them)
//   dsp_size alone   the whole AM / SAM detector (setSize_amd writes the size and nothing else, amd.c:253-256); gen0's phases and
//                    positions, the pulse flushed (setSize_gen, gen.c:369-373)
//   both             anf / anr's lidx and ngamma (flush_anf / flush_anr), snba's frame memory (calc_snba does not make it)
// State of a stage that is made on first use waits in `carry` for the allocation that makes the stage again.
int Engine::rebuild(int new_in, int new_dsp, int new_out, int new_size, int new_D)
{
    if (int rc = quiesce()) return rc;
    if (disp_fed_pending) QH_HIP(hipEventSynchronize(disp_fed));
    const bool rate = new_dsp != dsp_rate, size = new_size != dsp_size;
    struct Line { double2 *hist[2] = { nullptr, nullptr }; int cur = 0; std::vector<Fircore::Chan> chan; long long bytes = 0; } line[FC_COUNT];
    if (!size)
        for (int s : { (int)FC_NBP, (int)FC_BP1, (int)FC_DE, (int)FC_AUD, (int)FC_EQP }) {
            Fircore &f = fc[s];
            if (!f.hist[0] || f.parts > 1) continue;
            Line &l = line[s];
            l.cur = f.cur; l.chan = f.chan; l.bytes = owned[f.hist[0]];
            for (Fircore::Chan &r : l.chan) r.long_live = false;
            for (int i = 0; i < 2; i++) { l.hist[i] = f.hist[i]; owned.erase(f.hist[i]); f.hist[i] = nullptr; }
        }
    // the AM / SAM detector: setSize_amd keeps all of it; init_amd (a new dsp_rate) zeroes the loop and the two averages and leaves the
    // sideband all-pass chains (amd.c:72-113 writes no a[], b[], c[], d[], dsI, dsQ)
    AmState *am_keep = nullptr;
    PllState *pll_keep = nullptr;
    if (demod_alloc) { am_keep = am_state; pll_keep = pll_state; owned.erase(am_state); owned.erase(pll_state); am_state = nullptr; pll_state = nullptr; }
    // the stages made on first use: what is on the device now, or what an earlier rebuild left waiting for a stage not made since
    Carry keep = std::move(carry);
    for (int f = 0; f < 2; f++)
        if (lms_state[f]) {
            keep.lms[f].resize(2 * (size_t)nch);
            QH_HIP(hipMemcpy2D(keep.lms[f].data(), 2 * sizeof(double), &lms_state[f][0].lidx, sizeof(LmsState), 2 * sizeof(double), (size_t)nch, hipMemcpyDeviceToHost));
        }
    if (snba_state) {
        keep.snba_frames.resize((size_t)nch * 2 * kSnbX);
        QH_HIP(hipMemcpy2D(keep.snba_frames.data(), 2 * kSnbX * sizeof(double), snba_state, (size_t)snba_prm.state_doubles * sizeof(double),
                           2 * kSnbX * sizeof(double), (size_t)nch, hipMemcpyDeviceToHost));
    }
    if (rate) keep.gen.clear();         // calc_gen starts every phase again (gen.c:98-105,362-367)
    else if (gen_state) {
        keep.gen.resize((size_t)nch);
        QH_HIP(hipMemcpy(keep.gen.data(), gen_state, (size_t)nch * sizeof(GenState), hipMemcpyDeviceToHost));
        for (GenState &g : keep.gen) {  // flush_gen, as gen_flush_kernel: the pulse goes to OFF for as long as its state had left
            const long long pos = g.pulse_pos, up = gen_pnoff, on = up + gen_pntrans, down = on + gen_pnon, T = down + gen_pntrans;
            if (pos >= up) g.pulse_pos = (long long)gen_pnoff - ((pos < on ? on : pos < down ? down : T) - pos);
        }
    }
    std::vector<ChanCfg> keep_cfg;
    for (const ChanCfg &c : cfg) keep_cfg.push_back(settings_of(c, new_dsp));
    // the engine-wide settings (Engine::Wide) as a whole, and by hand the engine's identity and its count of replayed calls
    Wide was = std::move(wide);
    const int was_device = device, was_nch = nch;
    const hipStream_t was_stream = stream;
    const bool was_own_stream = own_stream;
    const unsigned long long was_epoch = epoch;
    const long long was_launches = graph_launches;
    own_stream = false;                     // the stream stays: callers hold it (qh_rxa_stream)
    this->~Engine();
    new (this) Engine();
    device = was_device; nch = was_nch; stream = was_stream; own_stream = was_own_stream; epoch = was_epoch + 1;
    in_rate = new_in; dsp_rate = new_dsp; out_rate = new_out; dsp_size = new_size; D = new_D;
    int rc = init();
    wide = std::move(was);
    graph_launches = was_launches;
    snba_tune_dirty = true;
    carry = std::move(keep);
    if (!rc) {
        cfg = keep_cfg;
        lists_dirty = true; eq_lists_dirty = true;
    }
    for (int s = 0; s < FC_COUNT; s++) {
        Line &l = line[s];
        if (!l.hist[0]) continue;
        Fircore &f = fc[s];
        for (int i = 0; i < 2; i++) { release(f.hist[i]); f.hist[i] = l.hist[i]; owned[l.hist[i]] = l.bytes; }
        f.cur = l.cur; f.chan = l.chan;
        f.carried = !f.mask;                // a stage init() has not made keeps the lines through the fc_alloc that makes it
    }
    if (am_keep) {
        if (!rc) rc = demod_init();
        if (!rc && !rate) {
            QH_HIP(hipMemcpyAsync(am_state, am_keep, (size_t)nch * sizeof(AmState), hipMemcpyDeviceToDevice, stream));
            QH_HIP(hipMemcpyAsync(pll_state, pll_keep, (size_t)nch * sizeof(PllState), hipMemcpyDeviceToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
        } else if (!rc) {
            const size_t at = offsetof(PllState, dsI);
            QH_HIP(hipMemcpy2DAsync(reinterpret_cast<char *>(pll_state) + at, sizeof(PllState), reinterpret_cast<const char *>(pll_keep) + at, sizeof(PllState),
                                    sizeof(PllState) - at, (size_t)nch, hipMemcpyDeviceToDevice, stream));
            QH_HIP(hipStreamSynchronize(stream));
        }
        (void)hipFree(am_keep); (void)hipFree(pll_keep);
    }
    if (rc) return rc;
    QH_HIP(hipStreamSynchronize(stream));
    return QH_OK;
}

}  // namespace qh
