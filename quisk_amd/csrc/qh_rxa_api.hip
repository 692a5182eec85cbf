// qh_rxa_api.hip -- the C ABI of the RXA engine (include/quiskhip.h, group 1): argument checks, the engine lock, setters that edit the
// host-side settings and mark them dirty, getters and diagnostics, host staging.  It launches no kernel and designs no filter: work on
// the device goes through Engine (qh_engine.hip, qh_engine_params.hip).
#include "qh_engine.hpp"

using namespace qh;

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
    int D = 0;
    if (nch <= 0) {
        set_error(QH_ERR_INVALID, "qh_rxa_create: bad arguments");
        return nullptr;
    }
    if (check_rates("qh_rxa_create", dsp_size, in_rate, dsp_rate, out_rate, &D)) return nullptr;
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
int qh_rxa_in_rate(const qh_rxa *h) { return h ? h->e.in_rate : 0; }
int qh_rxa_dsp_rate(const qh_rxa *h) { return h ? h->e.dsp_rate : 0; }
int qh_rxa_out_rate(const qh_rxa *h) { return h ? h->e.out_rate : 0; }
int qh_rxa_dsp_size(const qh_rxa *h) { return h ? h->e.dsp_size : 0; }

// The run-time setters of wdsp/channel.c:169-258 on a live engine: Engine::set_rates under the engine lock.  A value < 0 stands for the
// current one.  A call that changes nothing does nothing (`if (x != ch[channel].x)`, channel.c:172,185,201,215,231,245): the captured
// launch sequences stay.  A refused call sets the status qh_rxa_create would and changes nothing.
static int set_rates_locked(qh_rxa *h, int in_rate, int dsp_rate, int out_rate, int dsp_size)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    const Engine &e = h->e;
    return h->e.set_rates(in_rate < 0 ? e.in_rate : in_rate, dsp_rate < 0 ? e.dsp_rate : dsp_rate, out_rate < 0 ? e.out_rate : out_rate,
                          dsp_size < 0 ? e.dsp_size : dsp_size);
}
int qh_rxa_set_rates(qh_rxa *h, int in_rate, int dsp_rate, int out_rate)
{
    if (in_rate < 0 || dsp_rate < 0 || out_rate < 0) return set_error(QH_ERR_INVALID, "qh_rxa_set_rates: bad arguments");
    return set_rates_locked(h, in_rate, dsp_rate, out_rate, -1);
}
int qh_rxa_set_in_rate(qh_rxa *h, int in_rate) { return in_rate < 0 ? set_error(QH_ERR_INVALID, "qh_rxa_set_in_rate: bad arguments") : set_rates_locked(h, in_rate, -1, -1, -1); }
int qh_rxa_set_dsp_rate(qh_rxa *h, int dsp_rate) { return dsp_rate < 0 ? set_error(QH_ERR_INVALID, "qh_rxa_set_dsp_rate: bad arguments") : set_rates_locked(h, -1, dsp_rate, -1, -1); }
int qh_rxa_set_out_rate(qh_rxa *h, int out_rate) { return out_rate < 0 ? set_error(QH_ERR_INVALID, "qh_rxa_set_out_rate: bad arguments") : set_rates_locked(h, -1, -1, out_rate, -1); }
int qh_rxa_set_dsp_size(qh_rxa *h, int dsp_size) { return dsp_size < 0 ? set_error(QH_ERR_INVALID, "qh_rxa_set_dsp_size: bad arguments") : set_rates_locked(h, -1, -1, -1, dsp_size); }

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
    if (c.bp1_gain != gain) { c.bp1_gain = gain; c.w.bp1_dirty = true; }
}
static void bp1_set(ChanCfg &c)
{
    const int old = c.bp1_run;
    c.bp1_run = (c.amd_run || c.lms[0].run || c.lms[1].run || c.emnr_run || c.snba_run) ? 1 : 0;
    if (old != c.bp1_run) c.w.bp1_dirty = true;
    if (!old && c.bp1_run) c.w.bp1_flush = true;
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
            c.w.snb_dirty = true;
            c.w.epi_dirty = true;
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
            c.w.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}

int qh_rxa_SetRXABandpassFreqs(qh_rxa *h, int ch, double f_low, double f_high)
{
    FOR_CH(h, ch, {
        if (f_low != c.bp1_flow || f_high != c.bp1_fhigh) { c.bp1_flow = f_low; c.bp1_fhigh = f_high; c.w.bp1_dirty = true; }
    });
}

int qh_rxa_RXANBPSetFreqs(qh_rxa *h, int ch, double flow, double fhigh)
{
    FOR_CH(h, ch, {
        if (flow != c.nbp_flow || fhigh != c.nbp_fhigh) { c.nbp_flow = flow; c.nbp_fhigh = fhigh; c.w.nbp_dirty = true; }
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
            c.w.snba_taps_dirty = true; c.w.snba_rout_flush = true;
            c.w.epi_dirty = true;
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
    for (int c = ch < 0 ? 0 : ch; c < (ch < 0 ? h->e.nch : ch + 1); c++) apply(h->e.wide.snba_tune_h[(size_t)c], v);
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
    for (ChanCfg &c : h->e.cfg) { c.snba_f_low = 200.0; c.snba_f_high = 0.0; c.w.snba_taps_dirty = true; }
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
            c.w.snb_dirty = true;
            c.w.epi_dirty = true;
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

// What every fircore's nc setter takes: a power of two in [dsp_size, kLongNcMax].  who: the setter's name, heading the message of its
// QH_ERR_INVALID; none: RXASetNC and SetRXAFMSQNC, which answer QH_ERR_UNSUPPORTED.
static int nc_check(const qh_rxa *h, const char *who, int nc)
{
    if (nc >= 1 && !(nc & (nc - 1)) && nc <= kLongNcMax && !(h && nc < h->e.dsp_size)) return QH_OK;
    if (!who) return set_error(QH_ERR_UNSUPPORTED, "nc must be a power of two in [dsp_size, %d]", kLongNcMax);
    return set_error(QH_ERR_INVALID, "%s: nc must be a power of two in [dsp_size, %d]", who, kLongNcMax);
}

// xfmd's de-emphasis and audio filters, per channel (fmd.c:278-384).  Each acts only on a changed value, as there; the design rows follow
// at the next process call (Engine::fm_filters).  which: 0 the de-emphasis filter, 1 the audio filter.
static void fm_set_nc(Engine &e, ChanCfg &c, int which, int nc)
{
    int &cur = which ? c.fm_nc_aud : c.fm_nc_de;
    if (cur == nc) return;
    cur = nc;
    // setNc_fircore zeroes that filter's delay line (firmin.c:455-467): nothing long is held any more
    (which ? c.w.fm_aud_flush : c.w.fm_de_flush) = true;
    e.fc[which ? FC_AUD : FC_DE].chan[(size_t)(&c - e.cfg.data())].long_live = false;
    e.fm_dirty = true;
    if (!which) e.lists_dirty = true;       // the de-emphasis stage's channel pairs follow the designs
}
static void fm_set_mp(Engine &e, ChanCfg &c, int which, int mp)
{
    int &cur = which ? c.fm_mp_aud : c.fm_mp_de;
    if (cur == mp) return;
    cur = mp;                               // setMp_fircore: new masks, the line kept
    e.fm_dirty = true;
    if (!which) e.lists_dirty = true;
}
int qh_rxa_SetRXAFMNCde(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, "SetRXAFMNCde", nc)) return rc;
    FOR_CH(h, ch, { fm_set_nc(h->e, c, 0, nc); });
}
int qh_rxa_SetRXAFMNCaud(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, "SetRXAFMNCaud", nc)) return rc;
    FOR_CH(h, ch, { fm_set_nc(h->e, c, 1, nc); });
}
int qh_rxa_SetRXAFMMPde(qh_rxa *h, int ch, int mp) { FOR_CH(h, ch, { fm_set_mp(h->e, c, 0, mp ? 1 : 0); }); }
int qh_rxa_SetRXAFMMPaud(qh_rxa *h, int ch, int mp) { FOR_CH(h, ch, { fm_set_mp(h->e, c, 1, mp ? 1 : 0); }); }
// SetRXAFMAFFilter (fmd.c:364-384): both filters designed again, both delay lines kept (setImpulse_fircore)
int qh_rxa_SetRXAFMAFFilter(qh_rxa *h, int ch, double low, double high)
{
    if (!std::isfinite(low) || !std::isfinite(high)) return set_error(QH_ERR_INVALID, "SetRXAFMAFFilter: %g .. %g is not finite", low, high);
    if (low <= 0.0) return set_error(QH_ERR_INVALID, "SetRXAFMAFFilter: low %g must be above 0 (the de-emphasis curve takes log10(high / low))", low);
    if (high <= low) return set_error(QH_ERR_INVALID, "SetRXAFMAFFilter: high %g must be above low %g", high, low);
    FOR_CH(h, ch, {
        if (c.fm_f_low != low || c.fm_f_high != high) {
            c.fm_f_low = low; c.fm_f_high = high;
            h->e.fm_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}
// diagnostics: the design rows of the two filters on the device and the rows designed on the host since the engine was made
int qh_rxa_debug_fm_rows(qh_rxa *h, int *de_rows, int *aud_rows, long long *designed)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (de_rows) *de_rows = (int)h->e.fm_rows[0].size();
    if (aud_rows) *aud_rows = (int)h->e.fm_rows[1].size();
    if (designed) *designed = h->e.fm_designed;
    return QH_OK;
}

// nbp0's, bpsnba's and bp1's nc, mp and window, per stage (nbp.c:563-588, snb.c:829-855, bandpass.c:411-457).  Each acts only on a changed
// value, as there.  A new nc zeroes that stage's delay line and nothing long is held any more (setNc_fircore, firmin.c:454-466); a new mp
// or window designs the masks again and keeps the line (setMp_fircore, setImpulse_fircore).  which: FC_NBP, FC_SNB or FC_BP1.
static void band_set_nc(Engine &e, ChanCfg &c, int which, int nc)
{
    int &cur = which == FC_NBP ? c.nbp_nc : which == FC_SNB ? c.snb_nc : c.bp1_nc;
    if (cur == nc) return;
    cur = nc;
    (which == FC_NBP ? c.w.nbp_dirty : which == FC_SNB ? c.w.snb_dirty : c.w.bp1_dirty) = true;
    (which == FC_NBP ? c.w.nbp_flush : which == FC_SNB ? c.w.snb_flush : c.w.bp1_flush) = true;
    e.fc[which].chan[(size_t)(&c - e.cfg.data())].long_live = false;
}
static void band_set_mp(ChanCfg &c, int which, int mp)
{
    int &cur = which == FC_NBP ? c.nbp_mp : which == FC_SNB ? c.snb_mp : c.bp1_mp;
    if (cur == mp) return;
    cur = mp;
    (which == FC_NBP ? c.w.nbp_dirty : which == FC_SNB ? c.w.snb_dirty : c.w.bp1_dirty) = true;
}
int qh_rxa_RXANBPSetNC(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, "RXANBPSetNC", nc)) return rc;
    FOR_CH(h, ch, { band_set_nc(h->e, c, FC_NBP, nc); });
}
int qh_rxa_RXABPSNBASetNC(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, "RXABPSNBASetNC", nc)) return rc;
    FOR_CH(h, ch, { band_set_nc(h->e, c, FC_SNB, nc); });
}
int qh_rxa_SetRXABandpassNC(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, "SetRXABandpassNC", nc)) return rc;
    FOR_CH(h, ch, { band_set_nc(h->e, c, FC_BP1, nc); });
}
int qh_rxa_RXANBPSetMP(qh_rxa *h, int ch, int mp) { FOR_CH(h, ch, { band_set_mp(c, FC_NBP, mp ? 1 : 0); }); }
int qh_rxa_RXABPSNBASetMP(qh_rxa *h, int ch, int mp) { FOR_CH(h, ch, { band_set_mp(c, FC_SNB, mp ? 1 : 0); }); }
int qh_rxa_SetRXABandpassMP(qh_rxa *h, int ch, int mp) { FOR_CH(h, ch, { band_set_mp(c, FC_BP1, mp ? 1 : 0); }); }
// (fir_bandpass knows the windows 0 and 1, fir.c:94-118: any other value is refused and changes nothing)
int qh_rxa_SetRXABandpassWindow(qh_rxa *h, int ch, int wintype)
{
    if (wintype != 0 && wintype != 1) return set_error(QH_ERR_INVALID, "SetRXABandpassWindow: wintype %d (0 or 1)", wintype);
    FOR_CH(h, ch, { if (c.bp1_wintype != wintype) { c.bp1_wintype = wintype; c.w.bp1_dirty = true; } });
}

int qh_rxa_RXASetNC(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, nullptr, nc)) return rc;
    FOR_CH(h, ch, {
        // RXANBPSetNC, RXABPSNBASetNC, SetRXABandpassNC, wdsp/RXA.c:938-940
        band_set_nc(h->e, c, FC_NBP, nc); band_set_nc(h->e, c, FC_SNB, nc); band_set_nc(h->e, c, FC_BP1, nc);
        fm_set_nc(h->e, c, 0, nc); fm_set_nc(h->e, c, 1, nc);       // SetRXAFMNCde / SetRXAFMNCaud, wdsp/RXA.c:943-944
        c.fmsq_nc = nc;                         // SetRXAFMSQNC, wdsp/RXA.c:942
        if (c.eqp_nc != nc) { c.eqp_nc = nc; c.w.eqp_dirty = true; c.w.eqp_flush = true; }      // SetRXAEQNC, wdsp/RXA.c:941
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
            if (c.fnfrun) c.w.nbp_dirty = true;
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
            if (c.fnfrun) c.w.nbp_dirty = true;
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
            if (c.fnfrun) c.w.nbp_dirty = true;
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

int qh_rxa_RXANBPSetTuneFrequency(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { if (f != c.ndb_tunefreq) { c.ndb_tunefreq = f; if (c.fnfrun) c.w.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetShiftFrequency(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { if (f != c.ndb_shift) { c.ndb_shift = f; if (c.fnfrun) c.w.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetNotchesRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { run = run ? 1 : 0; if (run != c.fnfrun) { c.fnfrun = run; c.w.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetWindow(qh_rxa *h, int ch, int wintype) { FOR_CH(h, ch, { if (c.nbp_wintype != wintype) { c.nbp_wintype = wintype; c.w.nbp_dirty = true; } }); }
int qh_rxa_RXANBPSetAutoIncrease(qh_rxa *h, int ch, int autoincr) { FOR_CH(h, ch, { if (c.autoincr != autoincr) { c.autoincr = autoincr; if (c.fnfrun) c.w.nbp_dirty = true; } }); }

// RXASetMP (wdsp/RXA.c:948-958): minimum-phase impulse responses in every fircore of the channel's chain.
int qh_rxa_RXASetMP(qh_rxa *h, int ch, int mp)
{
    mp = mp ? 1 : 0;
    FOR_CH(h, ch, {
        // RXANBPSetMP, RXABPSNBASetMP, SetRXABandpassMP, wdsp/RXA.c:951-953
        band_set_mp(c, FC_NBP, mp); band_set_mp(c, FC_SNB, mp); band_set_mp(c, FC_BP1, mp);
        fm_set_mp(h->e, c, 0, mp); fm_set_mp(h->e, c, 1, mp);       // SetRXAFMMPde / SetRXAFMMPaud, wdsp/RXA.c:956-957
        c.fmsq_mp = mp;                         // SetRXAFMSQMP, wdsp/RXA.c:955
        if (c.eqp_mp != mp) { c.eqp_mp = mp; c.w.eqp_dirty = true; }      // SetRXAEQMP, wdsp/RXA.c:954
    });
}

int qh_rxa_SetRXAShiftRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.shift_run = run; c.w.nco_dirty = true; }); }
int qh_rxa_SetRXAShiftFreq(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { c.shift_freq = f; c.w.nco_dirty = true; }); }
int qh_rxa_RXANBPSetRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { if (c.nbp_run != run) { c.nbp_run = run; c.w.nbp_dirty = true; } }); }
// (bandpass.c:385-390 writes the flag and nothing else; where a fixed AGC gain is applied -- at the AGC's own spot or in the output matrix --
// depends on it: fix_before)
int qh_rxa_SetRXABandpassRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { if (c.bp1_run != run) { c.bp1_run = run; c.w.bp1_dirty = true; c.w.epi_dirty = true; h->e.lists_dirty = true; } }); }
int qh_rxa_SetRXAAMDSBMode(qh_rxa *h, int ch, int sbmode) { FOR_CH(h, ch, { c.sbmode = sbmode; c.w.demod_dirty = true; }); }
int qh_rxa_SetRXAAMDFadeLevel(qh_rxa *h, int ch, int levelfade) { FOR_CH(h, ch, { c.levelfade = levelfade; c.w.demod_dirty = true; }); }
int qh_rxa_SetRXAFMDeviation(qh_rxa *h, int ch, double deviation) { FOR_CH(h, ch, { c.fm_dev = deviation; c.w.demod_dirty = true; }); }
int qh_rxa_SetRXACTCSSFreq(qh_rxa *h, int ch, double freq) { FOR_CH(h, ch, { c.ctcss_freq = freq; c.w.demod_dirty = true; c.w.ctcss_flush = true; }); }
int qh_rxa_SetRXACTCSSRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.ctcss_run = run; c.w.demod_dirty = true; }); }
// SetRXAFMLimRun / SetRXAFMLimGain (wdsp/fmd.c:336-362): the FM detector's limiter
int qh_rxa_SetRXAFMLimRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { run = run ? 1 : 0; if (c.lim_run != run) { c.lim_run = run; h->e.lists_dirty = true; } }); }
int qh_rxa_SetRXAFMLimGain(qh_rxa *h, int ch, double gaindB)
{
    const double gain = std::pow(10.0, gaindB / 20.0);
    FOR_CH(h, ch, { if (c.lim_gain != gain) { c.lim_gain = gain; c.w.lim_dirty = true; } });
}

// SetRXAEMNRRun ... SetRXAEMNRPosition, wdsp/emnr.c:1096-1143
int qh_rxa_SetRXAEMNRRun(qh_rxa *h, int ch, int run)
{
    if (h && run && !h->e.wide.emnr_tables)
        return set_error(QH_ERR_INVALID, "EMNR needs its gain tables first (qh_rxa_SetEMNRTables: WDSP's `calculus` and `zetaHat.bin` data)");
    if (h && run && h->e.dsp_size > kEmnrIncr) return set_error(QH_ERR_UNSUPPORTED, "EMNR: dsp_size up to %d", kEmnrIncr);
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.emnr_run != run) {
            bp1_check_set(c, c.amd_run, c.lms[0].run, c.lms[1].run, run);
            c.emnr_run = run;
            bp1_set(c);
            c.w.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}
int qh_rxa_SetRXAEMNRgainMethod(qh_rxa *h, int ch, int method) { FOR_CH(h, ch, { c.emnr_gain_method = method; c.w.emnr_dirty = true; }); }
int qh_rxa_SetRXAEMNRnpeMethod(qh_rxa *h, int ch, int method) { FOR_CH(h, ch, { c.emnr_npe = method; c.w.emnr_dirty = true; }); }
int qh_rxa_SetRXAEMNRaeRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.emnr_ae = run ? 1 : 0; c.w.emnr_dirty = true; }); }
int qh_rxa_SetRXAEMNRaeZetaThresh(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_ae_zeta = v; c.w.emnr_dirty = true; }); }       // emnr.c:1145
int qh_rxa_SetRXAEMNRaePsi(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_ae_psi = v; c.w.emnr_dirty = true; }); }               // emnr.c:1153
int qh_rxa_SetRXAEMNRtrainZetaThresh(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_train_zeta = v; c.w.emnr_dirty = true; }); }  // emnr.c:1161
int qh_rxa_SetRXAEMNRtrainT2(qh_rxa *h, int ch, double v) { FOR_CH(h, ch, { c.emnr_train_t2 = v; c.w.emnr_dirty = true; }); }            // emnr.c:1169
int qh_rxa_SetRXAEMNRPosition(qh_rxa *h, int ch, int position)
{
    FOR_CH(h, ch, { c.emnr_pos = position ? 1 : 0; c.bp1_pos = position ? 1 : 0; c.w.epi_dirty = true; h->e.lists_dirty = true; });
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
    e.wide.h_GG.assign(GG, GG + 241 * 241); e.wide.h_GGS.assign(GGS, GGS + 241 * 241);
    e.wide.h_zeta.assign(zeta_hat, zeta_hat + 3600); e.wide.h_zeta_true.assign(zeta_true, zeta_true + 3600);
    e.wide.h_zrange[0] = gamma_min; e.wide.h_zrange[1] = gamma_max; e.wide.h_zrange[2] = xi_min; e.wide.h_zrange[3] = xi_max;
    e.wide.emnr_tables = true;
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
            c.w.lms[which].flush = true;
            c.w.lms[0].dirty = c.w.lms[1].dirty = true; c.w.epi_dirty = true;
            h->e.lists_dirty = true;
        }
    });
}
static int lms_vals(qh_rxa *h, int ch, int which, const int *taps, const int *delay, const double *gain, const double *leakage)
{
    // n_taps above ANF_DLINE_SIZE has the reference write past w[]; its mask would fold a delay outside the line, which no client means
    const bool bad_taps = taps && (*taps < 1 || *taps > kLmsLine);
    if (bad_taps || (delay && (*delay < 0 || *delay > kLmsLine - 1)))
        return set_error(QH_ERR_INVALID, "%s: %s %d (taps 1..%d, delay 0..%d)", which ? "ANR" : "ANF", bad_taps ? "taps" : "delay", bad_taps ? *taps : *delay,
                         kLmsLine, kLmsLine - 1);
    FOR_CH(h, ch, {
        ChanCfg::Lms &m = c.lms[which];
        const ChanCfg::Lms was = m;
        if (taps) m.taps = *taps;
        if (delay) m.delay = *delay;
        // the channel moves between lms_kernel's list and the long form's, or to another K of the long form
        if (Engine::lms_long_form(was) != Engine::lms_long_form(m) || (Engine::lms_long_form(m) && lms_long_K(was.taps) != lms_long_K(m.taps)))
            h->e.lists_dirty = true;
        if (gain) m.two_mu = *gain;
        if (leakage) m.gamma = *leakage;
        c.w.lms[which].flush = c.w.lms[which].dirty = true;
    });
}
static int lms_position(qh_rxa *h, int ch, int which, int position)
{
    FOR_CH(h, ch, {
        c.lms[which].position = position ? 1 : 0;
        c.bp1_pos = position ? 1 : 0;                 // "rxa[channel].bp1.p->position = position", anf.c:236
        c.w.lms[which].flush = true;
        c.w.lms[0].dirty = c.w.lms[1].dirty = true; c.w.epi_dirty = true;
        h->e.lists_dirty = true;
    });
}
// SetRXAAMSQRun / Threshold / MaxTail, wdsp/amsq.c:216-243
int qh_rxa_SetRXAAMSQRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { c.amsq_run = run ? 1 : 0; h->e.lists_dirty = true; }); }
int qh_rxa_SetRXAAMSQThreshold(qh_rxa *h, int ch, double threshold)
{
    FOR_CH(h, ch, { const double t = std::pow(10.0, threshold / 20.0); c.amsq_tail_thresh = 0.9 * t; c.amsq_unmute_thresh = t; c.w.amsq_dirty = true; });
}
int qh_rxa_SetRXAAMSQMaxTail(qh_rxa *h, int ch, double tail) { FOR_CH(h, ch, { c.amsq_max_tail = tail < 0.0 ? 0.0 : tail; c.w.amsq_dirty = true; }); }
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
        c.w.epi_dirty = true; c.w.agc_dirty = true; c.w.lms[0].dirty = c.w.lms[1].dirty = true; h->e.lists_dirty = true;
    });
}
int qh_rxa_SetRXAAGCAttack(qh_rxa *h, int ch, int attack_ms) { FOR_CH(h, ch, { c.agc_tau_attack = (double)attack_ms / 1000.0; c.w.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCDecay(qh_rxa *h, int ch, int decay_ms) { FOR_CH(h, ch, { c.agc_tau_decay = (double)decay_ms / 1000.0; c.w.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCHang(qh_rxa *h, int ch, int hang_ms) { FOR_CH(h, ch, { c.agc_hangtime = (double)hang_ms / 1000.0; c.w.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCTop(qh_rxa *h, int ch, double max_agc_db) { FOR_CH(h, ch, { c.agc_max_gain = std::pow(10.0, max_agc_db / 20.0); c.w.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCSlope(qh_rxa *h, int ch, int slope) { FOR_CH(h, ch, { c.agc_var_gain = std::pow(10.0, (double)slope / 20.0 / 10.0); c.w.agc_dirty = true; }); }
int qh_rxa_SetRXAAGCHangThreshold(qh_rxa *h, int ch, int t) { FOR_CH(h, ch, { c.agc_hang_thresh = (double)t / 100.0; c.w.agc_dirty = true; }); }

int qh_rxa_SetRXAAGCFixed(qh_rxa *h, int ch, double db)
{
    FOR_CH(h, ch, { c.agc_fixed = std::pow(10.0, db / 20.0); c.w.epi_dirty = true; c.w.lms[0].dirty = c.w.lms[1].dirty = true; });
}

// ---- the AGC's display-side knobs (wcpAGC.c:440-557): host arithmetic on what loadWcpAGC derives (wcpAGC.c:115-146).  Every setter of
// the reference ends in loadWcpAGC, so the derived values are functions of the channel's current settings: out_target from create_rxa's
// out_targ 1.0 and n_tau 4 (RXA.c:335-358), in loadWcpAGC's order of expressions.  The getters read the settings under the engine's lock
// and touch neither the device nor the stream.
static double agc_out_target() { return 1.0 * (1.0 - std::exp(-4.0)) * 0.9999; }
static double agc_min_volts(const ChanCfg &c) { return agc_out_target() / (c.agc_var_gain * c.agc_max_gain); }
static double agc_hang_level(const ChanCfg &c)
{
    const double tmp = std::pow(10.0, (c.agc_hang_thresh - 1.0) / 0.125);
    return (c.agc_max_input * tmp + (agc_out_target() / (c.agc_var_gain * c.agc_max_gain)) * (1.0 - tmp)) * 0.637;
}
// 10 log10((nbp0.fhigh - nbp0.flow) size / rate) of Get / SetRXAAGCThresh: size and rate are the caller's display FFT size and rate.
// The reference checks nothing and would take the log of 0 or less: refused here.
static int agc_noise_offset(const char *who, const ChanCfg &c, double size, double rate, double *offset)
{
    if (!std::isfinite(size) || !std::isfinite(rate) || size <= 0.0 || rate <= 0.0)
        return set_error(QH_ERR_INVALID, "%s: size %g and rate %g must be finite and above 0", who, size, rate);
    if (!(c.nbp_fhigh - c.nbp_flow > 0.0))
        return set_error(QH_ERR_INVALID, "%s: nbp0's band %g .. %g is not wider than 0", who, c.nbp_flow, c.nbp_fhigh);
    *offset = 10.0 * std::log10((c.nbp_fhigh - c.nbp_flow) * size / rate);
    return QH_OK;
}
// a getter's channel: one channel, not -1
static const ChanCfg *agc_get_chan(qh_rxa *h, int ch, const void *out, const char *who)
{
    if (!h || !out || ch < 0 || ch >= h->e.nch) { set_error(QH_ERR_INVALID, "%s: bad arguments", who); return nullptr; }
    return &h->e.cfg[(size_t)ch];
}
int qh_rxa_SetRXAAGCThresh(qh_rxa *h, int ch, double thresh, double size, double rate)
{
    if (!std::isfinite(thresh)) return set_error(QH_ERR_INVALID, "SetRXAAGCThresh: thresh %g is not finite", thresh);
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (ch < -1 || ch >= h->e.nch) return set_error(QH_ERR_INVALID, "channel %d out of range", ch);
    // every channel's value first: a refusal changes nothing
    const int lo = ch < 0 ? 0 : ch, hi = ch < 0 ? h->e.nch : ch + 1;
    std::vector<double> gain((size_t)(hi - lo));
    for (int i = lo; i < hi; i++) {
        const ChanCfg &c = h->e.cfg[(size_t)i];
        double noise_offset = 0.0;
        if (int rc = agc_noise_offset("SetRXAAGCThresh", c, size, rate, &noise_offset)) return rc;
        const double g = agc_out_target() / (c.agc_var_gain * std::pow(10.0, (thresh + noise_offset) / 20.0));
        if (!std::isfinite(g) || g <= 0.0) return set_error(QH_ERR_INVALID, "SetRXAAGCThresh: thresh %g gives no finite gain", thresh);
        gain[(size_t)(i - lo)] = g;
    }
    FOR_CH(h, ch, { c.agc_max_gain = gain[(size_t)(_i - _lo)]; c.w.agc_dirty = true; });
}
int qh_rxa_GetRXAAGCThresh(qh_rxa *h, int ch, double *thresh, double size, double rate)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    const ChanCfg *c = agc_get_chan(h, ch, thresh, "GetRXAAGCThresh");
    if (!c) return QH_ERR_INVALID;
    double noise_offset = 0.0;
    if (int rc = agc_noise_offset("GetRXAAGCThresh", *c, size, rate, &noise_offset)) return rc;
    *thresh = 20.0 * std::log10(agc_min_volts(*c)) - noise_offset;
    return QH_OK;
}
int qh_rxa_SetRXAAGCHangLevel(qh_rxa *h, int ch, double hang_level)
{
    if (!std::isfinite(hang_level)) return set_error(QH_ERR_INVALID, "SetRXAAGCHangLevel: level %g is not finite", hang_level);
    FOR_CH(h, ch, {
        const double min_volts = agc_min_volts(c);
        if (c.agc_max_input > min_volts) {
            const double convert = std::pow(10.0, hang_level / 20.0);
            const double tmp = std::max(1e-8, (convert - min_volts) / (c.agc_max_input - min_volts));
            c.agc_hang_thresh = 1.0 + 0.125 * std::log10(tmp);
        } else c.agc_hang_thresh = 1.0;
        c.w.agc_dirty = true;
    });
}
int qh_rxa_GetRXAAGCHangLevel(qh_rxa *h, int ch, double *hang_level)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    const ChanCfg *c = agc_get_chan(h, ch, hang_level, "GetRXAAGCHangLevel");
    if (!c) return QH_ERR_INVALID;
    *hang_level = 20.0 * std::log10(agc_hang_level(*c) / 0.637);
    return QH_OK;
}
int qh_rxa_GetRXAAGCHangThreshold(qh_rxa *h, int ch, int *hangthreshold)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    const ChanCfg *c = agc_get_chan(h, ch, hangthreshold, "GetRXAAGCHangThreshold");
    if (!c) return QH_ERR_INVALID;
    *hangthreshold = (int)(100.0 * c->agc_hang_thresh);
    return QH_OK;
}
int qh_rxa_GetRXAAGCTop(qh_rxa *h, int ch, double *max_agc)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    const ChanCfg *c = agc_get_chan(h, ch, max_agc, "GetRXAAGCTop");
    if (!c) return QH_ERR_INVALID;
    *max_agc = 20.0 * std::log10(c->agc_max_gain);
    return QH_OK;
}
int qh_rxa_SetRXAAGCMaxInputLevel(qh_rxa *h, int ch, double level)
{
    if (!std::isfinite(level) || level <= 0.0) return set_error(QH_ERR_INVALID, "SetRXAAGCMaxInputLevel: level %g must be finite and above 0", level);
    FOR_CH(h, ch, { c.agc_max_input = level; c.w.agc_dirty = true; });
}

// xcbl / xspeak / xmpeak.  Run flags, npeaks and the enables do not flush (cblock.c:120-126, iir.c:322-330, :490-515); the design
// setters recompute and zero their cascade -- speak's, or that one peak's (calc_speak ends in flush_speak, iir.c:216, :332-360, :517-548).
// npeaks outside [0, 2] and fil outside [0, 2) would index past the reference's two-peak arrays: refused, nothing changes.
static void ap_run_set(qh_rxa *h, ChanCfg &c, int &flag, int run)
{
    run = run ? 1 : 0;
    if (flag == run) return;
    flag = run;
    c.w.ap_dirty = true; c.w.epi_dirty = true;          // fix_before() follows ap_on()
    h->e.lists_dirty = true;
}
int qh_rxa_SetRXACBLRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { ap_run_set(h, c, c.cbl_run, run); }); }
int qh_rxa_SetRXASPCWRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { ap_run_set(h, c, c.sp_run, run); }); }
int qh_rxa_SetRXASPCWFreq(qh_rxa *h, int ch, double f) { FOR_CH(h, ch, { c.sp_f = f < 200.0 ? 200.0 : f; c.w.ap_dirty = true; c.w.sp_flush = true; }); }
int qh_rxa_SetRXASPCWBandwidth(qh_rxa *h, int ch, double bw) { FOR_CH(h, ch, { c.sp_bw = bw; c.w.ap_dirty = true; c.w.sp_flush = true; }); }
int qh_rxa_SetRXASPCWGain(qh_rxa *h, int ch, double g) { FOR_CH(h, ch, { c.sp_gain = g; c.w.ap_dirty = true; c.w.sp_flush = true; }); }
int qh_rxa_SetRXAmpeakRun(qh_rxa *h, int ch, int run) { FOR_CH(h, ch, { ap_run_set(h, c, c.mp_run, run); }); }
int qh_rxa_SetRXAmpeakNpeaks(qh_rxa *h, int ch, int npeaks)
{
    if (npeaks < 0 || npeaks > kApPeaks) return set_error(QH_ERR_INVALID, "SetRXAmpeakNpeaks: npeaks %d outside [0, %d]", npeaks, kApPeaks);
    FOR_CH(h, ch, { if (c.mp_npeaks != npeaks) { c.mp_npeaks = npeaks; c.w.ap_dirty = true; } });
}
int qh_rxa_SetRXAmpeakFilEnable(qh_rxa *h, int ch, int fil, int enable)
{
    if (fil < 0 || fil >= kApPeaks) return set_error(QH_ERR_INVALID, "SetRXAmpeakFilEnable: fil %d outside [0, %d)", fil, kApPeaks);
    FOR_CH(h, ch, { enable = enable ? 1 : 0; if (c.mp_enable[fil] != enable) { c.mp_enable[fil] = enable; c.w.ap_dirty = true; } });
}
static int mpeak_design(qh_rxa *h, int ch, int fil, int what, double v)
{
    if (fil < 0 || fil >= kApPeaks) return set_error(QH_ERR_INVALID, "SetRXAmpeakFil*: fil %d outside [0, %d)", fil, kApPeaks);
    FOR_CH(h, ch, {
        if (what == 0) c.mp_f[fil] = v < 200.0 ? 200.0 : v;
        else if (what == 1) c.mp_bw[fil] = v;
        else c.mp_gain[fil] = v;
        c.w.ap_dirty = true; c.w.mp_flush[fil] = true;
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
        if (c.ssql_run != run) { c.ssql_run = run; c.w.ssql_dirty = true; c.w.epi_dirty = true; h->e.lists_dirty = true; }   // fix_before() follows
    });
}
int qh_rxa_SetRXASSQLThreshold(qh_rxa *h, int ch, double threshold)
{
    if (!std::isfinite(threshold)) return set_error(QH_ERR_INVALID, "SetRXASSQLThreshold: threshold %g is not finite", threshold);
    FOR_CH(h, ch, { c.ssql_wthresh = threshold / 2.0; c.w.ssql_dirty = true; });
}
int qh_rxa_SetRXASSQLTauMute(qh_rxa *h, int ch, double tau)
{
    if (!std::isfinite(tau) || tau < 0.0) return set_error(QH_ERR_INVALID, "SetRXASSQLTauMute: tau %g is negative or not finite", tau);
    FOR_CH(h, ch, { c.ssql_tau_mute = tau; c.w.ssql_dirty = true; });
}
int qh_rxa_SetRXASSQLTauUnMute(qh_rxa *h, int ch, double tau)
{
    if (!std::isfinite(tau) || tau < 0.0) return set_error(QH_ERR_INVALID, "SetRXASSQLTauUnMute: tau %g is negative or not finite", tau);
    FOR_CH(h, ch, { c.ssql_tau_unmute = tau; c.w.ssql_dirty = true; });
}

// xfmsq (fmsq.c:235-279).  The noise filter's nc and mp are taken up at the next process call (one design for the engine's FMSQ
// channels); nothing here flushes the averages or the state machine, as there.
int qh_rxa_SetRXAFMSQRun(qh_rxa *h, int ch, int run)
{
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.fmsq_run != run) { c.fmsq_run = run; h->e.lists_dirty = true; }
    });
}
int qh_rxa_SetRXAFMSQThreshold(qh_rxa *h, int ch, double threshold)
{
    if (!std::isfinite(threshold)) return set_error(QH_ERR_INVALID, "SetRXAFMSQThreshold: threshold %g is not finite", threshold);
    FOR_CH(h, ch, { c.fmsq_tail_thresh = threshold; c.fmsq_unmute_thresh = 0.9 * threshold; c.w.fmsq_dirty = true; });
}
int qh_rxa_SetRXAFMSQNC(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, nullptr, nc)) return rc;
    FOR_CH(h, ch, { c.fmsq_nc = nc; });
}
int qh_rxa_SetRXAFMSQMP(qh_rxa *h, int ch, int mp) { FOR_CH(h, ch, { c.fmsq_mp = mp ? 1 : 0; }); }

// xeqp (eq.c:242-377).  A setter edits the channel's settings; the design is made on the host at the next process call (Engine::refresh_eqp).
int qh_rxa_SetRXAEQRun(qh_rxa *h, int ch, int run)
{
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.eqp_run != run) { c.eqp_run = run; h->e.eq_lists_dirty = true; }
    });
}
int qh_rxa_SetRXAEQNC(qh_rxa *h, int ch, int nc)
{
    if (int rc = nc_check(h, "SetRXAEQNC", nc)) return rc;
    FOR_CH(h, ch, { if (c.eqp_nc != nc) { c.eqp_nc = nc; c.w.eqp_dirty = true; c.w.eqp_flush = true; } });
}
int qh_rxa_SetRXAEQMP(qh_rxa *h, int ch, int mp)
{
    FOR_CH(h, ch, { mp = mp ? 1 : 0; if (c.eqp_mp != mp) { c.eqp_mp = mp; c.w.eqp_dirty = true; } });
}
static int eqp_set_profile(qh_rxa *h, int ch, int nfreqs, const double *F, const double *G, int ctfmode)
{
    if (!F || !G) return set_error(QH_ERR_INVALID, "EQ profile: null pointer");
    if (nfreqs < 1) return set_error(QH_ERR_INVALID, "EQ profile: nfreqs = %d", nfreqs);
    if (!std::isfinite(G[0])) return set_error(QH_ERR_INVALID, "EQ profile: the preamp gain is not finite");
    for (int i = 1; i <= nfreqs; i++)
        if (!std::isfinite(F[i]) || !std::isfinite(G[i])) return set_error(QH_ERR_INVALID, "EQ profile: point %d is not finite", i);
    std::vector<double> f(F, F + nfreqs + 1), g(G, G + nfreqs + 1);
    f[0] = 0.0;     // (not read by eq_impulse)
    FOR_CH(h, ch, {
        c.eqp_F = f; c.eqp_G = g;
        if (ctfmode >= 0) c.eqp_ctfmode = ctfmode;
        c.w.eqp_tie = eqp_profile_tie(f, g, (double)h->e.dsp_rate);
        c.w.eqp_dirty = true;
    });
}
int qh_rxa_SetRXAEQProfile(qh_rxa *h, int ch, int nfreqs, const double *F, const double *G) { return eqp_set_profile(h, ch, nfreqs, F, G, -1); }
int qh_rxa_SetRXAEQCtfmode(qh_rxa *h, int ch, int mode) { FOR_CH(h, ch, { c.eqp_ctfmode = mode; c.w.eqp_dirty = true; }); }
int qh_rxa_SetRXAEQWintype(qh_rxa *h, int ch, int wintype) { FOR_CH(h, ch, { c.eqp_wintype = wintype; c.w.eqp_dirty = true; }); }
int qh_rxa_SetRXAGrphEQ(qh_rxa *h, int ch, const int *rxeq)
{
    if (!rxeq) return set_error(QH_ERR_INVALID, "SetRXAGrphEQ: null pointer");
    const double F[5] = { 0.0, 150.0, 400.0, 1500.0, 6000.0 };
    const double G[5] = { (double)rxeq[0], (double)rxeq[1], (double)rxeq[1], (double)rxeq[2], (double)rxeq[3] };
    return eqp_set_profile(h, ch, 4, F, G, 0);
}
int qh_rxa_SetRXAGrphEQ10(qh_rxa *h, int ch, const int *rxeq)
{
    if (!rxeq) return set_error(QH_ERR_INVALID, "SetRXAGrphEQ10: null pointer");
    const double F[11] = { 0.0, 32.0, 63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 16000.0 };
    double G[11];
    for (int i = 0; i <= 10; i++) G[i] = (double)rxeq[i];
    return eqp_set_profile(h, ch, 10, F, G, 0);
}

int qh_rxa_SetRXAPanelGain1(qh_rxa *h, int ch, double g) { FOR_CH(h, ch, { c.gain1 = g; c.w.epi_dirty = true; }); }
int qh_rxa_SetRXAPanelGain2(qh_rxa *h, int ch, double gI, double gQ) { FOR_CH(h, ch, { c.gain2I = gI; c.gain2Q = gQ; c.w.epi_dirty = true; }); }
int qh_rxa_SetRXAPanelSelect(qh_rxa *h, int ch, int s) { FOR_CH(h, ch, { c.inselect = s; c.w.epi_dirty = true; }); }
int qh_rxa_SetRXAPanelCopy(qh_rxa *h, int ch, int cp) { FOR_CH(h, ch, { c.copy = cp; c.w.epi_dirty = true; }); }
// SetRXAPanelPan (patchpanel.c:158-176): the fields SetRXAPanelGain2 writes, by the reference's sine law (its PI, comm.h:146)
int qh_rxa_SetRXAPanelPan(qh_rxa *h, int ch, double pan)
{
    if (!std::isfinite(pan)) return set_error(QH_ERR_INVALID, "SetRXAPanelPan: pan %g is not finite", pan);
    const double PI = 3.1415926535897932;
    const double gain1 = pan <= 0.5 ? 1.0 : std::sin(pan * PI), gain2 = pan <= 0.5 ? std::sin(pan * PI) : 1.0;
    FOR_CH(h, ch, { c.gain2I = gain1; c.gain2Q = gain2; c.w.epi_dirty = true; });
}
// SetRXAPanelBinaural (patchpanel.c:186-192)
int qh_rxa_SetRXAPanelBinaural(qh_rxa *h, int ch, int bin) { FOR_CH(h, ch, { c.copy = 1 - bin; c.w.epi_dirty = true; }); }

int qh_rxa_process(qh_rxa *h, const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    if (!d_in || !d_out) return set_error(QH_ERR_INVALID, "null buffer");
    if (in_stride < (long long)nblk * h->e.dsp_insize || out_stride < (long long)nblk * h->e.dsp_outsize)
        return set_error(QH_ERR_INVALID, "stride shorter than nblk blocks");
    return h->e.process_fed(h->e.wide.graph_on, d_in, in_stride, d_out, out_stride, nblk);
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
    const int rc = h->e.process_fed(false, d_in, in_stride, nullptr, 0, nblk);
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
    launch_egress_pack(reinterpret_cast<const double2 *>(d_src), src_stride, nch, n, f, (hipStream_t)stream);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

int qh_rxa_set_graph_replay(qh_rxa *h, int on)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    h->e.wide.graph_on = on != 0;
    if (!on) { h->e.drop_graphs(); h->e.graph_key = Engine::GraphKey{}; }
    return QH_OK;
}
long long qh_rxa_graph_launches(const qh_rxa *h) { return h ? h->e.graph_launches : 0; }

int qh_rxa_set_band_tile(qh_rxa *h, int nfft)
{
    if (!h || (nfft != 0 && nfft != 4096 && nfft != 6144 && nfft != 8192)) return set_error(QH_ERR_INVALID, "qh_rxa_set_band_tile: 0 (default), 4096, 6144 or 8192");
    QH_RXA_LOCK(h);
    h->e.wide.band_tile_pref = nfft;
    h->e.epoch++;                   // the next call picks the tile anew (pick_band_tile): a captured launch sequence runs the old one
    return QH_OK;
}
int qh_rxa_band_tile(const qh_rxa *h) { return h ? h->e.bnfft : 0; }

int qh_rxa_set_snba_form(qh_rxa *h, int form)
{
    if (!h || (form != 0 && form != 1)) return set_error(QH_ERR_INVALID, "qh_rxa_set_snba_form: 0 (default) or 1 (the three passes wherever they can run)");
    QH_RXA_LOCK(h);
    h->e.wide.snba_form = form;
    h->e.epoch++;                   // a captured launch sequence runs the other form's kernels; the state is one layout for both
    return QH_OK;
}
int qh_rxa_snba_form(const qh_rxa *h) { return h ? h->e.wide.snba_form : 0; }

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
    const int rc = h->e.process_fed(false, reinterpret_cast<const double *>(d_src), (long long)nblk * h->e.dsp_insize, d_out, out_stride, nblk);
    h->e.pk_src = nullptr;
    return rc;
}

// flush_rxa (wdsp/RXA.c:527-559): NCO phase, resampler ring and fircore delay lines back to zero
int qh_rxa_flush(qh_rxa *h)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    return h->e.flush();
}

// ---- the data taps (qh_taps.hpp) -------------------------------------------------------------------------------------
// xsender's run && flag (sender.c:66-68) of channel ch, -1 = all: later calls leave the channel's signal behind nbp0 as float pairs
int qh_rxa_set_sender(qh_rxa *h, int ch, int run)
{
    if (h && h->e.wide.disp && !run) return set_error(QH_ERR_INVALID, "qh_rxa_set_sender: a display is attached (qh_rxa_attach_display), it reads every channel's rows");
    FOR_CH(h, ch, { run = run ? 1 : 0; if (c.sender_run != run) { c.sender_run = run; h->e.lists_dirty = true; } });
}

int qh_rxa_sender_rows(qh_rxa *h, const float **d_rows, long long *stride, int *n)
{
    if (!h || !d_rows || !stride || !n) return set_error(QH_ERR_INVALID, "qh_rxa_sender_rows: null argument");
    QH_RXA_LOCK(h);
    *d_rows = reinterpret_cast<const float *>(h->e.snd_rows); *stride = h->e.snd_cap; *n = (int)h->e.snd_n;
    return QH_OK;
}

int qh_rxa_sender_rows_host(qh_rxa *h, int ch, float *out, int max, int *n)
{
    if (!h || !out || !n) return set_error(QH_ERR_INVALID, "qh_rxa_sender_rows_host: null argument");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (ch < 0 || ch >= e.nch) return set_error(QH_ERR_INVALID, "channel %d out of range", ch);
    if (!e.cfg[(size_t)ch].sender_run) return set_error(QH_ERR_INVALID, "channel %d: the sender is off (qh_rxa_set_sender)", ch);
    *n = (int)e.snd_n;
    if (e.snd_n > max) return set_error(QH_ERR_INVALID, "qh_rxa_sender_rows_host: %lld samples, room for %d", e.snd_n, max);
    if (e.snd_n == 0) return QH_OK;
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipMemcpyAsync(out, e.snd_rows + (size_t)ch * (size_t)e.snd_cap, (size_t)e.snd_n * sizeof(float2), hipMemcpyDeviceToHost, e.stream));
    QH_HIP(hipStreamSynchronize(e.stream));
    return QH_OK;
}

// xsiphon's run (siphon.c:100) of channel ch, -1 = all.  A siphon that is switched on starts as flush_siphon leaves it (siphon.c:88-94).
int qh_rxa_set_siphon(qh_rxa *h, int ch, int run)
{
    FOR_CH(h, ch, {
        run = run ? 1 : 0;
        if (c.sip_run == run) continue;
        c.sip_run = run; h->e.lists_dirty = true;
        if (run && h->e.sip_ring) {
            QH_HIP(hipSetDevice(h->e.device));
            QH_HIP(hipMemsetAsync(h->e.sip_ring + (size_t)_i * kSipSize, 0, (size_t)kSipSize * sizeof(double2), h->e.stream));
            QH_HIP(hipMemsetAsync(h->e.sip_idx + _i, 0, sizeof(int), h->e.stream));
        }
    });
}

// suck (siphon.c:148-163) with outsize = size: the newest `size` samples, oldest first, as (I, Q) doubles.  The reference leaves sipout as
// it was when outsize > sipsize and its callers then read `size` samples of a sipsize buffer; here such a size is refused.
int qh_rxa_get_sip(qh_rxa *h, int ch, double *out, int size)
{
    if (!h || !out) return set_error(QH_ERR_INVALID, "qh_rxa_get_sip: null argument");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (ch < 0 || ch >= e.nch) return set_error(QH_ERR_INVALID, "channel %d out of range", ch);
    if (size < 0 || size > kSipSize) return set_error(QH_ERR_INVALID, "qh_rxa_get_sip: size %d outside 0 .. %d", size, kSipSize);
    if (!e.cfg[(size_t)ch].sip_run) return set_error(QH_ERR_INVALID, "channel %d: the siphon is off (qh_rxa_set_siphon)", ch);
    if (size == 0) return QH_OK;
    if (!e.sip_ring) { std::memset(out, 0, (size_t)size * 2 * sizeof(double)); return QH_OK; }      // no call since it was switched on
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipStreamSynchronize(e.stream));
    int idx = 0;
    QH_HIP(hipMemcpy(&idx, e.sip_idx + ch, sizeof(int), hipMemcpyDeviceToHost));
    const double2 *ring = e.sip_ring + (size_t)ch * kSipSize;
    const int j = (idx - size) & (kSipSize - 1), first = kSipSize - j < size ? kSipSize - j : size;
    QH_HIP(hipMemcpy(out, ring + j, (size_t)first * sizeof(double2), hipMemcpyDeviceToHost));
    if (first < size) QH_HIP(hipMemcpy(out + 2 * (size_t)first, ring, (size_t)(size - first) * sizeof(double2), hipMemcpyDeviceToHost));
    return QH_OK;
}

// The last call's sender rows to sub-span ss of a display bank, once (Engine::feed_display); every channel's sender must be on
int qh_rxa_feed_display(qh_rxa *h, qh_ana *a, int ss)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    return h->e.feed_display(a, ss);
}

// xsender -> Spectrum2 (sender.c:81) bank to bank: every later process call ends by feeding its sender rows to sub-span ss of a's
// displays, display d from channel d.  a = NULL detaches (the senders stay on).  The bank must outlive the attachment.
int qh_rxa_attach_display(qh_rxa *h, qh_ana *a, int ss)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (!a) { e.wide.disp = nullptr; return QH_OK; }
    if (qh_ana_ndisp(a) != e.nch || qh_ana_buff_size(a) != e.dsp_size || qh_ana_device(a) != e.device)
        return set_error(QH_ERR_INVALID, "qh_rxa_attach_display: the bank needs a display per channel (%d), buff_size = dsp_size (%d) and the engine's device",
                         e.nch, e.dsp_size);
    if (ss < 0 || ss >= qh_ana_num_stitch(a)) return set_error(QH_ERR_INVALID, "qh_rxa_attach_display: sub-span %d outside the bank's", ss);
    for (ChanCfg &c : e.cfg) if (!c.sender_run) { c.sender_run = 1; e.lists_dirty = true; }
    e.epoch++;
    e.wide.disp = a; e.wide.disp_ss = ss;
    return QH_OK;
}

// ---- gen0 (qh_gen.hpp): the SetRXAPreGen* setters of wdsp/gen.c:384-450 on (engine, channel), ch -1 = every channel -------------------
int qh_rxa_SetRXAPreGenRun(qh_rxa *h, int ch, int run)
{
    FOR_CH(h, ch, { run = run ? 1 : 0; if (c.gen_run != run) { c.gen_run = run; h->e.lists_dirty = true; } });
}
int qh_rxa_SetRXAPreGenMode(qh_rxa *h, int ch, int mode) { FOR_CH(h, ch, { c.gen_mode = mode; c.w.gen_dirty = true; }); }
int qh_rxa_SetRXAPreGenToneMag(qh_rxa *h, int ch, double mag) { FOR_CH(h, ch, { c.gen_tone_mag = mag; c.w.gen_dirty = true; }); }
// (calc_tone: the phase goes to 0, gen.c:31)
int qh_rxa_SetRXAPreGenToneFreq(qh_rxa *h, int ch, double freq) { FOR_CH(h, ch, { c.gen_tone_freq = freq; c.w.gen_tone_reset = true; c.w.gen_dirty = true; }); }
int qh_rxa_SetRXAPreGenNoiseMag(qh_rxa *h, int ch, double mag) { FOR_CH(h, ch, { c.gen_noise_mag = mag; c.w.gen_dirty = true; }); }
int qh_rxa_SetRXAPreGenSweepMag(qh_rxa *h, int ch, double mag) { FOR_CH(h, ch, { c.gen_sweep_mag = mag; c.w.gen_dirty = true; }); }
// (calc_sweep: the phase goes to 0 and dphs back to its start, gen.c:51-52)
int qh_rxa_SetRXAPreGenSweepFreq(qh_rxa *h, int ch, double freq1, double freq2)
{
    FOR_CH(h, ch, { c.gen_sweep_f1 = freq1; c.gen_sweep_f2 = freq2; c.w.gen_sweep_dirty = c.w.gen_sweep_reset = true; c.w.gen_dirty = true; });
}
int qh_rxa_SetRXAPreGenSweepRate(qh_rxa *h, int ch, double rate)
{
    FOR_CH(h, ch, { c.gen_sweep_rate = rate; c.w.gen_sweep_dirty = c.w.gen_sweep_reset = true; c.w.gen_dirty = true; });
}
// The seed of the channel's noise stream (the default is a fixed function of the channel); the stream goes on from the sample it has reached
int qh_rxa_set_gen_seed(qh_rxa *h, int ch, unsigned long long seed) { FOR_CH(h, ch, { c.gen_seed = seed; c.gen_seed_set = true; c.w.gen_dirty = true; }); }

// Meters (wdsp/meter.c): enable != 0 makes later process calls maintain the ADC, S and AGC meters.
int qh_rxa_enable_meters(qh_rxa *h, int enable)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    h->e.wide.meters_on = enable != 0;
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
    if (!e.wide.meters_on || !e.m_adc) { *value = -400.0; return QH_OK; }             // flush_meter's initial reading
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

// A diagnostics counter the kernels keep on the device, ctr[at]: 0 before it exists, else its value once everything enqueued has run
// (-1 when the device fails)
static long long read_counter(qh_rxa *h, int *Engine::*ctr, int at = 0)
{
    if (!h || !(h->e.*ctr)) return 0;
    QH_RXA_LOCK(h);
    int v = 0;
    if (hipSetDevice(h->e.device) != hipSuccess || hipStreamSynchronize(h->e.stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, h->e.*ctr + at, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

// Diagnostics of the time-tiled FM loop: tiles whose speculative warm-up had not converged and were re-run in order.
long long qh_rxa_pll_repairs(qh_rxa *h) { return read_counter(h, &Engine::pll_nfixed); }

// Diagnostics: check_only >= 0 sets the verify pass to count-only (1) or repair (0); then copies up to `max` doubles of
// channel ch's per-tile loop states of the last call ([tile][kPllEndsW]: pt, fil_out, omega where the warm-up ended / the tile ended).
int qh_rxa_debug_pll(qh_rxa *h, int check_only, int ch, double *out, int max)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (check_only >= 0) e.wide.pll_check_only = check_only;
    if (!out || max <= 0 || !e.pll_ends) return 0;
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipStreamSynchronize(e.stream));
    long long n = e.pll_ends_cap * kPllEndsW;
    if (n > max) n = max;
    QH_HIP(hipMemcpy(out, e.pll_ends + (long long)ch * e.pll_ends_cap * kPllEndsW, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return (int)n;
}

// Diagnostics: channel ch's FM squelch at the end of the last call: avnoise, longnoise, state (0 MUTED, 1 INCREASE, 2 UNMUTED, 3 TAIL,
// 4 DECREASE), count, ready.  Returns the doubles written (5), 0 while no channel of the engine has run the stage.
int qh_rxa_debug_fmsq(qh_rxa *h, int ch, double *out, int max)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (ch < 0 || ch >= e.nch) return set_error(QH_ERR_INVALID, "channel %d out of range", ch);
    if (!out || max < 5 || !e.fq_state) return 0;
    QH_HIP(hipSetDevice(e.device));
    QH_HIP(hipStreamSynchronize(e.stream));
    FmsqState st;
    QH_HIP(hipMemcpy(&st, e.fq_state + ch, sizeof(st), hipMemcpyDeviceToHost));
    out[0] = st.avnoise; out[1] = st.longnoise; out[2] = (double)st.state; out[3] = (double)st.count; out[4] = st.wait == 0 ? 1.0 : 0.0;
    return 5;
}

// Diagnostics: the complex taps behind the mask row channel ch's equalizer last got (eq_impulse, through mp_imp when mp is set; scale
// 1 / (2 dsp_size) as the reference's fircore gets them), kept on the host when the row was uploaded: 2 nc doubles.  A setter's new design
// shows here after the next process call in which the channel runs the stage, when the device holds it.  For a channel that has not run
// the stage yet (another channel of the engine has): what its current settings design.  Returns the number of taps, or 0 while no channel
// of the engine has run the stage or `max` is too small.
int qh_rxa_debug_eqp(qh_rxa *h, int ch, double *taps, int max)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    Engine &e = h->e;
    if (ch < 0 || ch >= e.nch) return set_error(QH_ERR_INVALID, "channel %d out of range", ch);
    const ChanCfg &c = e.cfg[(size_t)ch];
    if (!e.fc[FC_EQP].mask || !taps) return 0;
    const bool held = (size_t)ch < e.eq_taps_h.size() && !e.eq_taps_h[(size_t)ch].empty();
    if (!held && c.eqp_nc > kLongPart) return 0;
    const std::vector<cd> t = held ? e.eq_taps_h[(size_t)ch] : e.eqp_taps(c);
    if (max < 2 * (int)t.size()) return 0;
    std::memcpy(taps, t.data(), t.size() * sizeof(cd));
    return (int)t.size();
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
long long qh_rxa_agc_repairs(qh_rxa *h) { return read_counter(h, &Engine::agc_nfixed); }

// super-segments of the AGC boundary pass that were walked again (their warm-up had not ended on the true trajectory), over all calls
long long qh_rxa_agc_segments_rerun(qh_rxa *h) { return read_counter(h, &Engine::agc_nfixed, 1); }

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
    if (h->e.wide.agc_form != form) { h->e.wide.agc_form = form; h->e.drop_graphs(); h->e.epoch++; }
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

// The end of a host-fed call: the output rows go back to the host when the upload (err) and the call (rc) went well, everything enqueued
// is waited for and the device copies are freed.  The call's own status comes first, then the copies', then the wait's.
static int finish_host(Engine &e, int rc, hipError_t err, double *h_out, long long out_stride, long long n_out, void *din, double2 *dout)
{
    if (err == hipSuccess && rc == QH_OK)
        err = hipMemcpy2DAsync(h_out, (size_t)out_stride * sizeof(double2), dout, (size_t)n_out * sizeof(double2),
                               (size_t)n_out * sizeof(double2), (size_t)e.nch, hipMemcpyDeviceToHost, e.stream);
    hipError_t err2 = hipStreamSynchronize(e.stream);
    (void)hipFree(din); (void)hipFree(dout);
    if (rc != QH_OK) return rc;
    if (err != hipSuccess) return set_error(QH_ERR_HIP, "copy failed: %s", hipGetErrorString(err));
    if (err2 != hipSuccess) return set_error(QH_ERR_HIP, "synchronize failed: %s", hipGetErrorString(err2));
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
    if (dev_alloc(&dout, (size_t)e.nch * (size_t)n_out) != hipSuccess) { (void)hipFree(din); return set_error(QH_ERR_HIP, "hipMalloc failed"); }
    int rc = QH_OK;
    const hipError_t err = hipMemcpy2DAsync(din, (size_t)n_in * sizeof(double2), h_in, (size_t)in_stride * sizeof(double2),
                                            (size_t)n_in * sizeof(double2), (size_t)e.nch, hipMemcpyHostToDevice, e.stream);
    if (err == hipSuccess) rc = e.process_fed(false, reinterpret_cast<const double *>(din), n_in, reinterpret_cast<double *>(dout), n_out, nblk);
    return finish_host(e, rc, err, h_out, out_stride, n_out, din, dout);
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
    const hipError_t err = hipMemcpyAsync(dsrc, h_src, (size_t)src_bytes, hipMemcpyHostToDevice, e.stream);
    if (err == hipSuccess) rc = qh_rxa_process_packed(h, dsrc, src_bytes, fmt, chan_stride, reinterpret_cast<double *>(dout), n_out, nblk);
    return finish_host(e, rc, err, h_out, out_stride, n_out, dsrc, dout);
}

int qh_rxa_enable_timing(qh_rxa *h, int enable)
{
    if (!h) return set_error(QH_ERR_INVALID, "null engine");
    QH_RXA_LOCK(h);
    h->e.wide.timing = enable != 0;
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

namespace qh {
int rxa_gen_check(qh_rxa *h)
{
    if (!h) return QH_OK;
    QH_RXA_LOCK(h);
    for (const ChanCfg &c : h->e.cfg)
        if (c.gen_run && (c.gen_mode == 4 || c.gen_mode == 5))
            return set_error(QH_ERR_UNSUPPORTED, "channel %d: gen0 mode %d (%s) is not provided", (int)(&c - h->e.cfg.data()), c.gen_mode, c.gen_mode == 4 ? "sawtooth" : "triangle");
    return QH_OK;
}
}  // namespace qh
