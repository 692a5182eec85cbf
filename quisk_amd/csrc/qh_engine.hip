// qh_engine.hip -- the launch side of the RXA engine (qh_engine.hpp): process() and the stages of xrxa as kernel launches, the linear fast
// path and the per-mode path on channel lists, launch-sequence replay.  The front and nbp0 tile kernels the benchmark times are
// instantiated and launched here.  No setter, getter or design code belongs here (qh_rxa_api.hip, qh_engine_params.hip).
#include "qh_engine.hpp"

namespace qh {

void launch_egress_pack(const double2 *src, long long src_stride, int nch, long long n, const EgressFmt &f, hipStream_t s)
{
    const long long per = (n + 255) / 256;
    hipLaunchKernelGGL(egress_pack_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)nch), dim3(256), 0, s, src, src_stride,
                       (int)n, f);
}

void Engine::pack_audio(const double2 *src, long long src_stride, long long n)
{
    launch_egress_pack(src, src_stride, nch, n, eg, stream);
}

void Engine::tick(int cat)
{
    if (!wide.timing) return;
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
          int DET = 0, bool PAIR = false, bool MROW = false>
static void launch_osfir(OsfirArgs<double> a, int ntiles, int nch, hipStream_t s)
{
    a.ntiles = ntiles;
    dim3 grid((unsigned)ntiles * (unsigned)nch), block(NT);      // 1-D: the kernel maps ids to (channel, tile), qh_osfir.hpp
    constexpr int lds = osfir_lds_bytes<double, NFFT, D>();
    hipLaunchKernelGGL((osfir_kernel<double, NFFT, D, MIX, PACKED, METER, OUTMIX, EGRESS, POLY, DET, PAIR, MROW>), grid, block, lds, s, a);
}
// a stage that holds its mask rows by design (OsfirArgs::mask_row: the FM filters; no meters, no audio frames in their stores)
template <int NFFT>
static void launch_band_rows(OsfirArgs<double> a, int ntiles, int nch, hipStream_t s)
{
    launch_osfir<1, false, false, false, false, false, NFFT, false, 0, false, true>(a, ntiles, nch, s);
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
    if (a.mask_row) hipLaunchKernelGGL((osfir6k_kernel<false, false, true>), grid, block, lds, s, a);
    else if (meter && egress) hipLaunchKernelGGL((osfir6k_kernel<true, true>), grid, block, lds, s, a);
    else if (meter) hipLaunchKernelGGL((osfir6k_kernel<true, false>), grid, block, lds, s, a);
    else if (egress) hipLaunchKernelGGL((osfir6k_kernel<false, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((osfir6k_kernel<false, false>), grid, block, lds, s, a);
}

static void launch_band2g(OsfirArgs<double> a, int ntiles, int nch, hipStream_t s, bool meter, bool egress)
{
    a.ntiles = ntiles;
    dim3 grid((unsigned)ntiles * (unsigned)nch), block(kOsfir8kThreads);
    constexpr int lds = osfir8k_lds_bytes();
    if (a.mask_row) hipLaunchKernelGGL((osfir8k_kernel<false, false, true>), grid, block, lds, s, a);
    else if (meter && egress) hipLaunchKernelGGL((osfir8k_kernel<true, true>), grid, block, lds, s, a);
    else if (meter) hipLaunchKernelGGL((osfir8k_kernel<true, false>), grid, block, lds, s, a);
    else if (egress) hipLaunchKernelGGL((osfir8k_kernel<false, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((osfir8k_kernel<false, false>), grid, block, lds, s, a);
}

// The dynamic-LDS limits of this unit's tile kernels (Engine::init) and of emnr_kernel (Engine::emnr_alloc): an attribute belongs to the
// copy of a kernel that the unit it is set from emits, so they are set here, where the kernels are launched
int Engine::tile_lds_limits()
{
    // dynamic LDS of the overlap-save kernels
#define QH_SET_LDS(D, ...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir_kernel<double, 4096, D, __VA_ARGS__>), \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (osfir_lds_bytes<double, 4096, D>())))
    QH_SET_LDS(1, false); QH_SET_LDS(1, false, false, true);
    QH_SET_LDS(1, false, false, false, false, true); QH_SET_LDS(1, false, false, true, false, true);
    QH_SET_LDS(1, false, false, false, false, false, false, 0, false, true); QH_SET_LDS(1, false, false, false, false, false, false, 0, true, true);   // MROW, plain and PAIR
#define QH_SET_LDS8(...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir_kernel<double, kBandNfftMax, 1, false, false, __VA_ARGS__>), \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (osfir_lds_bytes<double, kBandNfftMax, 1>())))
    QH_SET_LDS8(false, false, false); QH_SET_LDS8(true, false, false); QH_SET_LDS8(false, false, true); QH_SET_LDS8(true, false, true);
    QH_SET_LDS8(false, false, false, false, 0, false, true);       // MROW
#undef QH_SET_LDS8
#define QH_SET_LDS6K(...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir6k_kernel<__VA_ARGS__>), \
        hipFuncAttributeMaxDynamicSharedMemorySize, osfir6k_lds_bytes()))
    QH_SET_LDS6K(false, false); QH_SET_LDS6K(true, false); QH_SET_LDS6K(false, true); QH_SET_LDS6K(true, true); QH_SET_LDS6K(false, false, true);
#undef QH_SET_LDS6K
#define QH_SET_LDS2G(...) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&osfir8k_kernel<__VA_ARGS__>), \
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, osfir8k_lds_bytes()))
    QH_SET_LDS2G(false, false); QH_SET_LDS2G(true, false); QH_SET_LDS2G(false, true); QH_SET_LDS2G(true, true); QH_SET_LDS2G(false, false, true);
#undef QH_SET_LDS2G
    QH_SET_LDS(2, false, false, false, true, false, true); QH_SET_LDS(4, false, false, false, true, false, true); QH_SET_LDS(8, false, false, false, true, false, true);
    QH_SET_LDS(2, false, true, false, true, false, true); QH_SET_LDS(4, false, true, false, true, false, true); QH_SET_LDS(8, false, true, false, true, false, true);
#undef QH_SET_LDS
    if (D > 1) QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&front_mask_kernel<kNfft>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (TileFft<kNfft, false, double2>::kLdsBytes)));
    return QH_OK;
}

int Engine::emnr_lds_limit()
{
    QH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&emnr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, emnr_lds_bytes()));
    return QH_OK;
}

// ---- the kernels of the parameter side (qh_engine_params.hip holds no device code: refresh_params and flush launch through these)
// the stored raw history of the first n channels of retune_list, re-expressed for their new phase laws (retune_law)
void Engine::launch_nco_retune(int n)
{
    hipLaunchKernelGGL(nco_retune_hist_kernel, dim3((kHistFront + NT - 1) / NT, (unsigned)n), dim3(NT), 0, stream,
                       hist_front[cur_front], kHistFront, nco_phase, nco_dphase, nco_parked, (const int *)retune_list,
                       (const unsigned long long *)retune_law);
}

void Engine::launch_nco_park(int ch, int run)
{
    hipLaunchKernelGGL(nco_park_kernel, dim3(1), dim3(1), 0, stream, nco_phase, nco_parked, ch, run);
}

// the modulated masks and phasor tables of the first n channels of retune_list
void Engine::launch_front_masks(int n)
{
    hipLaunchKernelGGL((front_mask_kernel<kNfft>), dim3((unsigned)n), dim3(NT), (size_t)(TileFft<kNfft, false, double2>::kLdsBytes),
                       stream, (const double *)front_taps, front_ntaps, (const unsigned long long *)nco_dphase, (const int *)retune_list, front_fold,
                       (const double2 *)tw4096, mask_front, lane_rot, nco_step, 1);
}

void Engine::launch_ssql_flush()
{
    hipLaunchKernelGGL(ssql_flush_kernel, dim3((unsigned)nch), dim3(64), 0, stream, ssql_state);
}

void Engine::launch_fmsq_flush()
{
    hipLaunchKernelGGL(fmsq_flush_kernel, dim3((unsigned)((nch + 63) / 64)), dim3(64), 0, stream, fq_state, nch, fq_nready);
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
// partition p is added only where the channel's own impulse response reaches it (row_parts: per mask row, row_stride 0 for a shared mask;
// mask_row: the channels' rows of a stage that holds them by design, else null)
static __global__ __launch_bounds__(NT) void long_add_kernel(double2 *dst, long long dst_stride, const double2 *add, long long add_stride, int n, const int *chan_list,
                                                             const int *row_parts, int row_stride, const int *mask_row, int p)
{
    const int ch = chan_list ? chan_list[blockIdx.y] : (int)blockIdx.y;
    if (p >= row_parts[mask_row ? (long long)mask_row[ch] : (long long)ch * row_stride]) return;
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

// one fircore stage (overlap-save, D = 1) over all channels (list == nullptr) or a sub-set: from the half f.cur of its delay lines to
// the other one.  The caller flips the pair (f.flip()) once it has run the stage over every list of the call.
void Engine::run_band(const double2 *src, long long src_stride, double2 *dst, long long dst_stride, const EpiParam *ep,
                      long long n_mid, Fircore &f, int P,
                      const int *list, int nlist, bool meter, bool egress, int det, double *det_out, long long det_stride,
                      const int *pairs, int npairs)
{
    const int hc = f.cur;
    double2 *const *hist = f.hist;
    if (f.parts > 1) {
        // nc > 4096: y = sum_p h_p * (x delayed by 4096 p).  lcat holds the stage's last 16383 samples and the block in one row per
        // channel, so partition p is the ordinary tile pass (4096 taps, 8192 points, 4097 outputs per tile) over a row that begins
        // 4096 p samples further back; the partitions' outputs are added, the epilogue follows as a pass of its own.  (The callers
        // switch every fusion off for such a call: no meters, audio frames or detector steps in this stage's stores.)
        const int K = f.parts, Pk = kLongPart - 1, Lk = kBandNfftMax - Pk, nt = (int)((n_mid + Lk - 1) / Lk);
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
        hipLaunchKernelGGL(long_gather_kernel, dim3((unsigned)(per < 2048 ? per : 2048), (unsigned)nl), dim3(NT), 0, stream, (const double2 *)f.lhist[hc], src,
                           src_stride, (int)n_mid, lcat, cat_stride, list, lh);
        for (int p = 0; p < K; p++) {
            OsfirArgs<double> a{};
            a.in = lcat + kLongHist - (long long)kLongPart * p; a.in_stride = cat_stride;
            a.hist = a.in - Pk; a.hist_stride = cat_stride; a.hist_len = Pk;
            a.out = p ? ltmp : dst; a.out_stride = p ? lcat_cap : dst_stride; a.out_offset = 0;
            a.mask = f.lmask + (size_t)p * kBandNfftMax; a.mask_stride = f.mask_stride ? (long long)kLongParts * kBandNfftMax : 0;
            a.mask_row = f.mask_row;
            a.tw_fwd = a.tw_inv = tw8192;
            a.tw_r2 = tw8192 + 32;
            a.chan_list = list;
            a.n_in = (int)n_mid; a.n_out = (int)n_mid; a.off = 0; a.P = Pk; a.Lout = Lk;
            if (f.mask_row) launch_band_rows<kBandNfftMax>(a, nt, nl, stream);
            else launch_band<kBandNfftMax>(a, nt, nl, stream, false, false);
            const long long pn = (n_mid + NT - 1) / NT;
            if (p) hipLaunchKernelGGL(long_add_kernel, dim3((unsigned)(pn < 1024 ? pn : 1024), (unsigned)nl), dim3(NT), 0, stream, dst, dst_stride,
                                      (const double2 *)ltmp, lcat_cap, (int)n_mid, list, (const int *)f.lrow_parts, f.mask_stride ? 1 : 0, (const int *)f.mask_row, p);
        }
        const long long pn = (n_mid + NT - 1) / NT;
        if (ep) hipLaunchKernelGGL((pointwise_kernel<double, false>), dim3((unsigned)(pn < 1024 ? pn : 1024), (unsigned)nl), dim3(NT), 0, stream,
                                   (const double2 *)dst, dst_stride, dst, dst_stride, (int)n_mid, (const unsigned long long *)nullptr,
                                   (const unsigned long long *)nullptr, ep, list);
        tick(2);
        hipLaunchKernelGGL(long_hist_kernel, dim3(64, (unsigned)nl), dim3(NT), 0, stream, (const double2 *)lcat, cat_stride, (int)n_mid, f.lhist[hc ^ 1], list, lh);
        return;
    }
    const int Lout = bnfft - P;
    const int ntiles = (int)((n_mid + Lout - 1) / Lout);
    OsfirArgs<double> a{};
    a.in = src; a.in_stride = src_stride;
    a.hist = hist[hc]; a.hist_stride = kHistBand; a.hist_len = kHistBand;
    a.out = dst; a.out_stride = dst_stride; a.out_offset = 0;
    a.mask = f.mask; a.mask_stride = f.mask_stride;
    a.mask_row = f.mask_row;                // null but for a stage with more than one design row (fm_filters)
    a.tw_fwd = a.tw_inv = (bnfft == kNfft || band2g) ? tw4096 : tw8192;
    a.tw_r2 = tw8192 + 32;                  // second pass table of the 8192-point plan: exp(-2 pi i k / 8192), k < 256 (qh_design.cpp)
    a.epi = ep;
    a.chan_list = list;
    a.n_in = (int)n_mid; a.n_out = (int)n_mid; a.off = 0; a.P = P; a.Lout = Lout;
    tick(1);
    if (meter) {            // the tables of Engine::meters_alloc
        const int lanes = band6k ? kOsfir6kThreads : NT;
        a.meter_in = m_part[0]; a.meter_out = m_part[1]; a.meter_stride = m_part_cap;
        a.meter_w = m_w + (band6k ? kMeterW384 : 0); a.meter_pk = m_w + kMeterPk;
        a.meter_mnt = std::exp(-(double)lanes / ((double)dsp_rate * 0.100));
        a.meter_sshift = __builtin_ctz((unsigned)dsp_size);
    }
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
        if (a.mask_row) launch_osfir<1, false, false, false, false, false, kNfft, false, 0, true, true>(a, ntiles, npairs, stream);
        else launch_osfir<1, false, false, false, false, false, kNfft, false, 0, true>(a, ntiles, npairs, stream);
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
    else if (a.mask_row && bnfft == kNfft) launch_band_rows<kNfft>(a, ntiles, nl, stream);
    else if (a.mask_row) launch_band_rows<kBandNfftMax>(a, ntiles, nl, stream);
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
        // the taps' points lie between stages: the per-mode path has them, as for the meters it cannot fuse (process_chain)
        if (c.sender_run || c.sip_run) k.mixed = k.taps = true;
        // gen0 writes between the front stage and the adc meter: the per-mode path has that point too.  The sawtooth's and the triangle's
        // wraps (`t += delta; if (t > period) t -= period`, gen.c:267-284) hang on the rounding of a sum that is not periodic, which only
        // the sequential chain reproduces; the reference marks both "audio only" and no RXA setter reaches their parameters: refused.
        if (c.gen_run) {
            if (c.gen_mode == 4 || c.gen_mode == 5)
                return set_error(QH_ERR_UNSUPPORTED, "channel %d: gen0 mode %d (%s) is not provided", (int)(&c - cfg.data()), c.gen_mode, c.gen_mode == 4 ? "sawtooth" : "triangle");
            k.mixed = k.gen = true;
        }
        if (c.ssql_on() && ((int)(0.070 * dsp_rate) < 64))
            return set_error(QH_ERR_UNSUPPORTED, "SSQL needs ramps of 64 samples or more: dsp_rate %d is too low", dsp_rate);
        if (c.emnr_run && !wide.emnr_tables) return set_error(QH_ERR_INVALID, "EMNR needs its gain tables first (qh_rxa_SetEMNRTables: WDSP's `calculus` and `zetaHat.bin` data)");
        if (c.nbp_run) { k.any_nbp = true; if (c.nbp_nc > k.nc_max) k.nc_max = c.nbp_nc; } else k.every_nbp = false;
        if (c.bp1_run) { k.any_bp1 = true; if (c.bp1_nc > k.nc_max) k.nc_max = c.bp1_nc; }
        if (c.snba_run && c.snb_nc > k.nc_max) k.nc_max = c.snb_nc;       // bpsnba's own nc (RXABPSNBASetNC)
        if (c.fmd_run) {
            k.nc_max = std::max({ k.nc_max, c.fm_nc_de, c.fm_nc_aud });
            // fir_bandpass's upper edge 1.1 f_high (fmd.c:115) and fc_impulse's grid need it below the Nyquist frequency
            if (1.1 * c.fm_f_high >= 0.5 * (double)dsp_rate)
                return set_error(QH_ERR_UNSUPPORTED, "channel %d: FM audio band up to %g Hz needs 1.1 * high below dsp_rate / 2 = %g", (int)(&c - cfg.data()),
                                 c.fm_f_high, 0.5 * (double)dsp_rate);
        }
        if (c.fmsq_run) {
            const int ch = (int)(&c - cfg.data());
            // (the reference would run its noise filter over the audio buffer xfmd last wrote, however long ago)
            if (!c.fmd_run) return set_error(QH_ERR_UNSUPPORTED, "channel %d: FMSQ runs while the FM detector is off", ch);
            // 2 F / rate of the design's upper two points would both clamp to 1.0 (eq.c:53-55) and the order qsort leaves them in is not defined
            if ((double)dsp_rate <= 2.0 * fm_pllpole(1.0, 20000.0))
                return set_error(QH_ERR_UNSUPPORTED, "FMSQ needs a dsp rate above twice the FM loop's pole frequency (%.0f Hz): %d is too low",
                                 2.0 * fm_pllpole(1.0, 20000.0), dsp_rate);
            if (c.fmsq_nc > kLongPart) return set_error(QH_ERR_UNSUPPORTED, "channel %d: FMSQ nc = %d exceeds %d", ch, c.fmsq_nc, kLongPart);
            if (c.fmsq_nc > k.nc_max) k.nc_max = c.fmsq_nc;
        }
    }
    for (const ChanCfg &c : cfg) {
        if (!c.eqp_run) continue;
        const int ch = (int)(&c - cfg.data());
        k.any_eqp = true;
        if (c.eqp_nc > kLongPart) return set_error(QH_ERR_UNSUPPORTED, "channel %d: EQ nc = %d exceeds %d", ch, c.eqp_nc, kLongPart);
        // qsort leaves the order of equal keys undefined (eq.c:53-63), and with it the design
        if (c.w.eqp_tie) return set_error(QH_ERR_UNSUPPORTED, "channel %d: two EQ frequencies coincide in [0, rate / 2] while their gains differ", ch);
        if (c.eqp_nc > k.nc_max) k.nc_max = c.eqp_nc;
    }
    {   // one noise filter design for the engine's FMSQ channels
        const ChanCfg *first = nullptr;
        for (const ChanCfg &c : cfg) {
            if (!c.fmsq_run) continue;
            if (first && (first->fmsq_nc != c.fmsq_nc || first->fmsq_mp != c.fmsq_mp))
                return set_error(QH_ERR_UNSUPPORTED, "FMSQ channels with different nc or mp in one engine");
            if (!first) first = &c;
        }
    }
    if (k.nc_max > kLongNcMax) return set_error(QH_ERR_UNSUPPORTED, "nc = %d exceeds %d", k.nc_max, kLongNcMax);
    return QH_OK;
}

// stages whose impulse response is longer than 4096 taps run in partitions (run_band): how many, per stage
int Engine::plan_long(ChainCall &k)
{
    auto parts = [](int nc) { return nc > kLongPart ? (nc + kLongPart - 1) / kLongPart : 1; };
    int lp[FC_COUNT];
    for (int &v : lp) v = 1;
    // Over every channel that runs the stage OR still holds a long delay line of it: a fircore keeps its delay line while it does not run (xbandpass / xnbp with run = 0
    // only copy; SetRXABandpassRun, a mode change back to AM / FM, RXANBPSetRun switch it on again without a flush), so a channel with
    // nc > 4096 that sits out holds 16383 samples the one-tile form has no room for.  Had the form followed the RUNNING channels,
    // the only long channel leaving took the stage to the short form (its line cut to 4095 samples) and came back to zeros behind
    // them: one long call 0.65 off (walk rxa_long 900190, found by round 6's seed sweep; in the suite since).
    // (long_live: the channel has run the stage with such an nc since RXASetNC last zeroed its lines.)
    // The FM pair takes its count from the larger of nc_de / nc_aud together; bpsnba goes by its own nc (RXABPSNBASetNC; RXASetNC keeps it at nbp0's).
    for (int ch = 0; ch < nch; ch++) {
        const ChanCfg &c = cfg[(size_t)ch];
        const int run[FC_COUNT] = { c.nbp_run, c.bp1_run, c.fmd_run, c.fmd_run, c.snba_run, 0, 0 };
        const int fm_nc = std::max(c.fm_nc_de, c.fm_nc_aud);
        const int nc[FC_COUNT] = { c.nbp_nc, c.bp1_nc, fm_nc, fm_nc, c.snb_nc, 0, 0 };
        for (int s = 0; s < FC_COUNT; s++) {
            if (!fc[s].can_long) continue;
            Fircore::Chan &r = fc[s].chan[(size_t)ch];
            if (run[s] && parts(nc[s]) > 1) r.long_live = true;
            if (run[s] || r.long_live) lp[s] = std::max(lp[s], parts(nc[s]));
        }
    }
    for (int s = 0; s < FC_COUNT; s++) {
        Fircore &f = fc[s];
        if (lp[s] > 1) { k.long_mode = true; if (int rc = long_stage_alloc(f)) return rc; }
        if (lp[s] == f.parts) continue;
        if (int rc = quiesce()) return rc;
        if ((lp[s] > 1) != (f.parts > 1)) {       // the delay lines move with the form
            // BOTH ping-pong halves: a channel that has left the stage's list (another mode, bp1 or SNBA switched off) keeps its rows in
            // the half that was current when it left (Fircore::Chan::at), which need not be the current one
            for (int half = 0; half < 2; half++)
                if (f.hist[half] && f.lhist[half])
                    hipLaunchKernelGGL(long_migrate_kernel, dim3(16, (unsigned)nch), dim3(NT), 0, stream, f.hist[half], f.lhist[half], lp[s] > 1 ? 1 : 0);
        }
        f.parts = lp[s];
        // the stage's masks are laid out for another form now: all of them again
        if (f.dirty) for (ChanCfg &c : cfg) c.w.*f.dirty = true;
        else fm_dirty = fm_relayout = true;     // (the FM pair's design rows)
    }
    return QH_OK;
}

// The fircore tile.  Impulse responses longer than 2048 taps need 8192 points (osfir_kernel<8192>, one wave per SIMD).
// Shorter ones run 4096-point tiles; the two-group 8192-point tile (osfir8k_kernel, 6144 instead of 2049 outputs per
// pair of transforms) is there on request (qh_rxa_set_band_tile) -- it measured slower, see qh_osfir.hpp.  The masks are
// spectra of the tile size, so a change rebuilds every one of them (the delay lines, kept 4095 samples deep, carry over).
void Engine::pick_band_tile(int nc_max)
{
    const bool two_group = nc_max <= 2048 && wide.band_tile_pref == 8192;
    const bool six_k = nc_max <= 2048 && wide.band_tile_pref == 6144;
    const int want = six_k ? kOsfir6kN : (nc_max > 2048 || two_group) ? kBandNfftMax : kNfft;
    if (want != bnfft || two_group != band2g || six_k != band6k) {
        bnfft = want; band2g = two_group; band6k = six_k;
        for (ChanCfg &c : cfg) { c.w.nbp_dirty = c.w.bp1_dirty = true; c.w.snb_dirty = true; }
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
    // bp1 does not, fixed AGC gain): the band tile then starts on a multiple of 256 samples, so that the 64 samples a wavefront
    // holds in one register lie in one DSP block and the taps' peak decay is scalar work (qh_osfir.hpp, "fused meters").  Any
    // other chain takes the per-mode path with the stand-alone meter kernel.
    k.meters_fused = wide.meters_on && !k.mixed && k.any_nbp && !k.any_bp1 && !k.any_eqp && dsp_size >= 64 && dsp_size <= 2048 && !k.long_mode;
    if (wide.meters_on && !k.meters_fused) k.mixed = true;
    if (wide.meters_on) if (int rc = meters_alloc()) return rc;
    if (int rc = refresh_params()) return rc;
    if (k.mixed) if (int rc = refresh_demod()) return rc;
    if (k.gen) if (int rc = refresh_gen()) return rc;
    // bp1 on the linear path (SetRXABandpassRun on an all-SSB engine): run_linear flips bp1's ping-pong pair like the per-mode path, but
    // refresh_lists, which tells bp1's record who runs it, is a step of refresh_demod only.  Left alone, the first per-mode call found no
    // channel listed and every line still at the half of the engine's first call, and after an odd number of linear calls copied that
    // stale half over the channel's current delay line (test_gpu_rxa_stage_combinations.py: `fmsq beside bp1`).
    if (!k.mixed && k.any_bp1) {
        std::vector<int> run;
        for (int ch = 0; ch < nch; ch++) if (cfg[(size_t)ch].bp1_run) run.push_back(ch);
        if (int rc = fc_follow(fc[FC_BP1], run)) return rc;
    }
    if (lists[L_SNBA].n) if (int rc = refresh_params()) return rc;       // bpsnba's mask needs the buffers the line above may just have made
    if (k.any_eqp || eq_lists_dirty) if (int rc = refresh_eqp()) return rc;

    k.n_in = (long long)nblk * dsp_insize;
    k.n_mid = (long long)nblk * dsp_size;
    if (k.n_in > 0x7fffffffLL) return set_error(QH_ERR_INVALID, "too many samples in one call");
    if (int rc = ensure_buffers(k.n_mid)) return rc;
    if (k.long_mode) if (int rc = long_buffers()) return rc;
    if (int rc = refresh_ap(k)) return rc;
    if (int rc = refresh_ssql(k)) return rc;
    // (snba_state: a linear call keeps the lists of the last per-mode one, and that one may have ended in snba_alloc's refusal, before any ratio was set)
    if (lists[L_SNBA].n && snba_state && snba_rows()) if (int rc = grow(snba_r12, snba_r12_cap, buf_cap / snba_prm.ratio, 2 * (long long)nch)) return rc;   // the blanker's 12 kHz rows
    if (fq_lists[0].n) if (int rc = grow(fq_noise, fq_noise_cap, buf_cap, nch)) return rc;     // the noise filter's output rows
    if (k.taps && tap_lists[0].n) if (int rc = grow(snd_rows, snd_cap, buf_cap, nch)) return rc;      // the sender's float rows
    snd_n = k.taps && tap_lists[0].n ? k.n_mid : 0;
    ev_used = 0;

    k.in = reinterpret_cast<const double2 *>(d_in); k.in_stride = in_stride;
    k.out = reinterpret_cast<double2 *>(d_out); k.out_stride = out_stride;
    // (with a partitioned stage in the call the others run 4096-tap tiles: their own nc is at most that)
    k.P = band6k ? kOsfir6kP : band2g ? kOsfir8kP : k.meters_fused ? ((k.nc_max - 1 + 255) / 256) * 256 : k.long_mode ? kLongPart - 1 : k.nc_max - 1;
    // audio egress (qh_rxa_process_audio): the narrowing rides in the store of the last kernel when that is an overlap-save
    // band stage or the per-mode path's output pass; other endings write complex doubles to the staging rows and narrow after
    k.eg_fused = eg.kind && (k.mixed ? lists[L_AMSQ].n == 0 : ((k.any_nbp || k.any_bp1 || k.any_eqp) && !k.long_mode));
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
    if (lists[L_SNB].n || lists[L_SNB + 1].n) fc[FC_SNB].flip();     // both positions' launches read the one half
    if (int rc = run_snba(k)) return rc;            // xsnba, RXA.c:578
    eqp_inplace(k);                                 // xeqp, RXA.c:579
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
    const int nstage = 1 + (k.any_nbp ? 1 : 0) + (k.any_eqp ? 1 : 0) + (k.any_bp1 ? 1 : 0);
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
    for (int f = 0; f < 3; f++) {       // xnbp, xeqp, xbandpass (RXA.c:568,579,582)
        if (f == 0 ? !k.any_nbp : f == 1 ? !k.any_eqp : !k.any_bp1) continue;
        long long dst_stride;
        double2 *dst = dst_of(stage, dst_stride);
        if (f == 1) {
            // the equalizer's channels through their tiles, each with its own mask and delay line; a channel that does not run it is
            // passed on as it is (xeqp with run 0 copies, eq.c:206-207, and its fircore's delay line stays as it was)
            const bool last = stage == nstage - 1;
            run_band(cur, cur_stride, dst, dst_stride, last ? epi : nullptr, n_mid, fc[FC_EQP], k.P, eq_lists[0].dev, eq_lists[0].n, false, k.eg_fused && last);
            fc[FC_EQP].flip();
            if (eq_lists[1].n) {
                const long long per = (n_mid + NT - 1) / NT;
                const dim3 g((unsigned)(per < 1024 ? per : 1024), (unsigned)eq_lists[1].n);
                if (!last) hipLaunchKernelGGL(copy_rows_kernel, g, dim3(NT), 0, stream, cur, dst, buf_cap, (int)n_mid, (const int *)eq_lists[1].dev);
                else {
                    auto *pass = k.eg_fused ? &pointwise_kernel<double, false, true> : &pointwise_kernel<double, false>;
                    hipLaunchKernelGGL(pass, g, dim3(NT), 0, stream, cur, cur_stride, dst, dst_stride, (int)n_mid, (const unsigned long long *)nullptr,
                                       (const unsigned long long *)nullptr, (const EpiParam *)epi, (const int *)eq_lists[1].dev, k.eg_fused ? eg : EgressFmt{});
                }
            }
            cur = dst; cur_stride = dst_stride; stage++;
            continue;
        }
        if (k.meters_fused) if (int rc = ensure_meter_partials(n_mid, bnfft - k.P)) return rc;
        Fircore &band = fc[f == 0 ? FC_NBP : FC_BP1];
        run_band(cur, cur_stride, dst, dst_stride, stage == nstage - 1 ? epi : nullptr, n_mid, band, k.P, nullptr, 0, k.meters_fused, k.eg_fused && stage == nstage - 1);
        band.flip();
        cur = dst; cur_stride = dst_stride; stage++;
    }
    if (k.meters_fused)
        hipLaunchKernelGGL(meter_finish_kernel, dim3((unsigned)nch), dim3(kMeterFinishThreads), 0, stream, m_part[0], m_part[1],
                           m_part_cap, (int)n_mid, dsp_size, bnfft - k.P, meter_parts(), m_adc, m_s, m_agc,
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
    k.split = lists[L_FM].n > 0 && lists[L_REST].n > 0 && D > 1 && !wide.meters_on && !k.taps && !k.gen && !lists[L_AMSQ].n && !lists[L_SNB].n && !wide.timing && !(dbg_forms & 1);
    // ... and when nothing sits between a channel's last filter and the output matrix (no AGC state machine, LMS, EMNR, SNBA,
    // limiter, squelch or position-1 stage anywhere), that last stage -- nbp0 for the plain channels, bp1 for AM / SAM, the CTCSS
    // notch for FM -- applies the matrix in its store and writes the caller's buffer: the output pass (32 B per output sample) goes.
    k.fm_theta_fused = k.split && k.any_nbp && !band6k && !band2g && bnfft == kNfft && !(dbg_forms & 8);
    bool no_lms = true;
    for (int f = 0; f < 2; f++) for (int p = 0; p < 3; p++) no_lms = no_lms && !lms_n(3 * f + p);
    k.direct = k.split && !(dbg_forms & 2) && !eq_lists[0].n && k.every_nbp && !eg.kind && !lists[L_LIM].n && !lists[L_AGC_CUR].n && !lists[L_AGC_OTHER].n && !lists[L_SNBA].n && !lists[L_SNB + 1].n && no_lms &&
               !lists[L_EMNR].n && !lists[L_EMNR + 1].n && !lists[L_EMNR + 2].n && !lists[L_FIX].n && !lists[L_FIX + 1].n && !lists[L_BP1P + 1].n && lists[L_BP1P].n == lists[L_BP1].n && lists[L_RB].n == lists[L_BP1].n &&
               lists[L_USB].n + lists[L_FM].n == lists[L_PLAIN].n && !lists[L_AP].n && !lists[L_AP + 1].n && !ssql_lists.any() &&
               // the first stores to `out` come while other channels' input is still being read: not for a caller that works in place
               extents_apart(k.out, k.out_stride, k.n_mid, k.in, k.in_stride, k.n_in, nch);
    // ... and the AM channels' nbp0 leaves the envelope and every tile's share of the fade leveller's averages: one pass does the rest
    k.P_am = ((k.P + 63) / 64) * 64;
    k.am_fused = k.direct && !(dbg_forms & 4) && lists[L_AM].n > 0 && lists[L_RB].n == lists[L_AM].n + lists[L_SAM].n && !band6k && !band2g && bnfft == kNfft && k.P_am < bnfft;
    // ... or, when the tiles are 2048 outputs behind 2048 samples of pre-roll and bp1 takes its channels two a tile, no pass at all: the
    // leveller's local share in nbp0's store (DET 3), the carried share in bp1's load
    k.am_lv_fused = k.am_fused && k.P_am == 2048 && bnfft - k.P_am == 2048 && np_am > 0 && lists[L_BP1P].n && fc[FC_BP1].parts <= 1 && !(dbg_forms & (16 | 512));
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
        // nbp0 over the lists of the two streams, each on its own channels' rows of the one half: the pair flips once, below
        Fircore &nbp = fc[FC_NBP];
        // the FM channels' nbp0 feeds the loop's phase detector and nothing else: its store takes the angles (first half of the rows)
        if (k.any_nbp) run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, nbp, P, lists[L_FM].dev, lists[L_FM].n, false, false,
                                k.fm_theta_fused ? 1 : 0, reinterpret_cast<double *>(other), 2 * buf_cap);
        if (fork_at >= 2) if (int rc = fork_side()) return rc;
        std::swap(stream, side_stream);
        int rc2 = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid, lists[L_REST].dev, lists[L_REST].n, 2);
        if (!rc2 && k.any_nbp) {
            if (k.direct) {     // the plain channels end here: output matrix in the store, straight to the caller's buffer
                if (lists[L_USB].n) run_band(cur, buf_cap, k.out, k.out_stride, epi, n_mid, nbp, P, lists[L_USB].dev, lists[L_USB].n);
                if (k.am_fused) {
                    if (lists[L_SAM].n) run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, nbp, P, lists[L_SAM].dev, lists[L_SAM].n);
                    run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, nbp, k.P_am, lists[L_AM].dev, lists[L_AM].n, false, false,
                             k.am_lv_fused ? 3 : 2, reinterpret_cast<double *>(other), 2 * buf_cap);
                } else if (lists[L_RB].n) run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, nbp, P, lists[L_RB].dev, lists[L_RB].n);
            } else run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, nbp, P, lists[L_REST].dev, lists[L_REST].n);
        }
        std::swap(stream, side_stream);
        if (rc2) return rc2;
        if (k.any_nbp) { nbp.flip(); std::swap(cur, other); }
        if (int rc = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid, nullptr, 0, 3)) return rc;          // histories, oscillator phases
    } else {
        if (int rc = run_front(k.in, k.in_stride, cur, buf_cap, nullptr, n_in, n_mid)) return rc;
        run_gen(k);                  // xgen (RXA.c:565)
        if (wide.meters_on) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)nch), dim3(64), 0, stream, cur, buf_cap, k.nblk, dsp_size, m_adc,
                                          m_prm, (const int *)nullptr);
        if (k.any_nbp) {
            run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, fc[FC_NBP], P, nullptr, 0);
            fc[FC_NBP].flip();
            std::swap(cur, other);
        }
    }
    if (wide.meters_on) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)nch), dim3(64), 0, stream, cur, buf_cap, k.nblk, dsp_size, m_s,
                                      m_prm, (const int *)nullptr);
    run_sender(k);                   // xsender (RXA.c:570)
    if (lists[L_AMSQ].n) {           // xamsqcap (RXA.c:571): the magnitudes of the signal behind nbp0, for xamsq at the end of the chain
        if (int rc = grow(amsq_mag, amsq_mag_cap, buf_cap, nch)) return rc;
        long long per = (n_mid + NT - 1) / NT;
        hipLaunchKernelGGL(amsq_cap_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)lists[L_AMSQ].n), dim3(NT), 0, stream, cur, buf_cap,
                           (int)n_mid, lists[L_AMSQ].dev, amsq_mag, amsq_mag_cap);
    }
    // xbpsnbaout at position 0 (RXA.c:572): the 250..5700 Hz filter of the signal ahead of nbp0 replaces nbp0's output
    if (lists[L_SNB].n) {
        if (k.any_nbp) run_band(other, buf_cap, cur, buf_cap, nullptr, n_mid, fc[FC_SNB], P, lists[L_SNB].dev, lists[L_SNB].n);
        else snb_inplace(k, lists[L_SNB].dev, lists[L_SNB].n);
    }
    tick(1);
    return QH_OK;
}

// bpsnba on the listed channels' rows of cur, through the rows of other (process_chain flips the stage's pair behind position 1)
void Engine::snb_inplace(const ChainCall &k, const int *list, int n)
{
    run_band(k.cur, buf_cap, k.other, buf_cap, nullptr, k.n_mid, fc[FC_SNB], k.P, list, n);
    long long per = (k.n_mid + NT - 1) / NT;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)n), dim3(NT), 0, stream, k.other, k.cur, buf_cap,
                       (int)k.n_mid, list);
}

// xeqp (RXA.c:579) on the listed channels' rows of cur, through the rows of other: every channel of the call lies in cur here, behind
// its detector, bpsnba and xsnba.  (The stores that write the caller's rows ahead of this point are off for such a call: plan_mixed.)
void Engine::eqp_inplace(const ChainCall &k)
{
    if (!eq_lists[0].n) return;
    run_band(k.cur, buf_cap, k.other, buf_cap, nullptr, k.n_mid, fc[FC_EQP], k.P, eq_lists[0].dev, eq_lists[0].n);
    fc[FC_EQP].flip();
    long long per = (k.n_mid + NT - 1) / NT;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)eq_lists[0].n), dim3(NT), 0, stream, k.other, k.cur, buf_cap,
                       (int)k.n_mid, (const int *)eq_lists[0].dev);
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
                               pll_nfixed, wide.pll_check_only);
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
        Fircore &bp1 = fc[FC_BP1];       // (run_output flips its pair)
        if (k.am_fused) {
            if (amlv_src.a) band_amlv = &amlv_src;
            run_band(other, buf_cap, k.out, k.out_stride, epi, n_mid, bp1, k.P, lists[L_AM].dev, lists[L_AM].n, false, false, 0, nullptr, 0,
                     np_am && !(dbg_forms & 16) ? lists[L_PAIRS_AM].dev : nullptr, np_am);
            band_amlv = nullptr;
            if (lists[L_SAM].n) run_band(cur, buf_cap, k.out, k.out_stride, epi, n_mid, bp1, k.P, lists[L_SAM].dev, lists[L_SAM].n, false, false, 0,
                                nullptr, 0, np_sam && !(dbg_forms & 16) ? lists[L_PAIRS_SAM].dev : nullptr, np_sam);
        } else run_band(cur, buf_cap, k.out, k.out_stride, epi, n_mid, bp1, k.P, lists[L_BP1P].dev, lists[L_BP1P].n);
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
    const bool fmdc_fused = pair && fc[FC_DE].parts <= 1 && !(dbg_forms & 256);
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
                           pll_nfixed, wide.pll_check_only, fmdc_fused ? 1 : 0);
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
    if (fq_lists[0].n) {
        // xfmsq's noise filter (fmsq.c:147) over the trigger, xfmd's audio ahead of de-emphasis (RXA.c:220): the FMSQ channels' rows only,
        // with the stage's own mask and delay lines.  Where the audio is made in the load (fmdc_fused) it is loaded the same way here, two
        // channels a tile (the taps are real); otherwise it lies in the rows of cur.
        if (fmdc_src.a) band_fmdc = &fmdc_src;
        run_band(cur, buf_cap, fq_noise, fq_noise_cap, nullptr, n_mid, fc[FC_FQ], k.P, fq_lists[0].dev, fq_lists[0].n, false, false, 0, nullptr, 0,
                 fmdc_src.a ? fq_lists[1].dev : nullptr, np_fq);
        fc[FC_FQ].flip();
        band_fmdc = nullptr;
    }
    {   // de-emphasis: real taps on a real signal, two channels per tile
        if (fmdc_src.a) band_fmdc = &fmdc_src;
        run_band(cur, buf_cap, other, buf_cap, nullptr, n_mid, fc[FC_DE], k.P, lists[L_FM].dev, lists[L_FM].n, false, false, 0, nullptr, 0,
                 pair ? lists[L_PAIRS_FM].dev : nullptr, np_fm);
        band_fmdc = nullptr;
    }
    run_band(other, buf_cap, cur, buf_cap, nullptr, n_mid, fc[FC_AUD], k.P, lists[L_FM].dev, lists[L_FM].n);   // audio filter
    // the pair's two stages run in every call of run_fm and flip together, here and nowhere else: their halves never differ
    fc[FC_DE].flip(); fc[FC_AUD].flip();
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
        hipLaunchKernelGGL(wide.agc_form == 1 ? wcpagc_seq_kernel : wcpagc_kernel, dim3((unsigned)lists[L_LIM].n), dim3(64), 0, stream, cur, buf_cap,
                           (int)n_mid, lists[L_LIM].dev, lim_prm, lim_state, 0.4);
    run_fmsq(k);            // xfmsq, RXA.c:575
    return QH_OK;
}

// The squelch of the listed FM channels behind xfmd: averages, state machine and gain in place on their rows of cur -- or, where the
// CTCSS notch has applied the output matrix and written the caller's rows (direct), on those: the gain is a real scalar on I and Q and
// commutes with the matrix, a muted sample is stored as 0 either way, and no other channel's path changes because one squelch runs.
void Engine::run_fmsq(const ChainCall &k)
{
    if (!fq_lists[0].n) return;
    hipLaunchKernelGGL(fmsq_kernel, dim3((unsigned)fq_lists[0].n), dim3(64), 0, stream, k.direct ? k.out : k.cur, k.direct ? k.out_stride : buf_cap, (int)k.n_mid,
                       (const int *)fq_lists[0].dev, (const double2 *)fq_noise, fq_noise_cap, (const FmsqParam *)fq_prm, fq_state, (const double *)fq_cup,
                       (const double *)fq_cdown);
}

// xsnba, with the tuning the setters left uploaded first
int Engine::run_snba(const ChainCall &k)
{
    if (!lists[L_SNBA].n) return QH_OK;
    if (snba_tune_dirty) {
        QH_HIP(hipMemcpyAsync(snba_tune, wide.snba_tune_h.data(), wide.snba_tune_h.size() * sizeof(SnbaTune), hipMemcpyHostToDevice, stream));
        QH_HIP(hipStreamSynchronize(stream));
        snba_tune_dirty = false;
    }
    const SnbaParam &q = snba_prm;
    const unsigned n = (unsigned)lists[L_SNBA].n;
    const int *list = lists[L_SNBA].dev;
    if (!snba_rows()) {
        hipLaunchKernelGGL(snba_kernel<false>, dim3(n), dim3(64), 0, stream, k.cur, buf_cap, k.nblk, dsp_size, list, q, snba_hin, snba_hout,
                           snba_state, snba_idx, snba_scratch, (const SnbaTune *)snba_tune, (const double *)nullptr, (double *)nullptr, 0LL);
        return QH_OK;
    }
    // the three passes: dsp_rate -> 12 kHz for the whole call, the frames on the 12 kHz rows, 12 kHz -> dsp_rate; each resampler's
    // history is written behind its pass, the input one's before the last pass overwrites the rows it is taken from
    const int n12 = k.nblk * q.isize, T = snba_decim_T(q.ratio), hin = q.cpp_in - 1, hout = q.cpp_out - 1;
    double *r_in = snba_r12, *r_out = snba_r12 + (long long)nch * snba_r12_cap;
    hipLaunchKernelGGL(snba_decim_kernel, dim3((unsigned)((n12 + T - 1) / T), n), dim3((unsigned)T), (size_t)snba_decim_lds_doubles(q.ratio, T) * sizeof(double), stream,
                       (const double2 *)k.cur, buf_cap, n12, list, q, (const double *)snba_hin, (const double *)snba_state, r_in, snba_r12_cap);
    if (hin) hipLaunchKernelGGL(snba_hist_kernel, dim3(n), dim3(256), (size_t)hin * sizeof(double), stream, (const double *)reinterpret_cast<double *>(k.cur),
                                2 * buf_cap, 2, (int)k.n_mid, list, snba_state, q.state_doubles, q.off_rin, hin);
    hipLaunchKernelGGL(snba_kernel<true>, dim3(n), dim3(64), 0, stream, k.cur, buf_cap, k.nblk, dsp_size, list, q, snba_hin, snba_hout,
                       snba_state, snba_idx, snba_scratch, (const SnbaTune *)snba_tune, (const double *)r_in, r_out, snba_r12_cap);
    hipLaunchKernelGGL(snba_interp_kernel, dim3((unsigned)((k.n_mid + 255) / 256), n), dim3(256), 0, stream, k.cur, buf_cap, n12, list, q,
                       (const double *)snba_hout, (const double *)snba_state, (const double *)r_out, snba_r12_cap);
    if (hout) hipLaunchKernelGGL(snba_hist_kernel, dim3(n), dim3(256), (size_t)hout * sizeof(double), stream, (const double *)r_out, snba_r12_cap, 1, n12, list,
                                 snba_state, q.state_doubles, q.off_rout, hout);
    return QH_OK;
}

// xanf and xanr of list entry pos ([f][0] position 0; [f][1 + b] position 1 with the data in cur / other), on the rows of b, and
// xemnr behind them (RXA.c:581,585)
void Engine::lms_at(const ChainCall &k, int pos, double2 *b)
{
    for (int f = 0; f < 2; f++)
        if (lists[L_LMS + 3 * f + pos].n) hipLaunchKernelGGL(lms_kernel, dim3((unsigned)lists[L_LMS + 3 * f + pos].n), dim3(64), 0, stream, b, buf_cap, (int)k.n_mid,
                                              lists[L_LMS + 3 * f + pos].dev, lms_prm[f], lms_state[f]);
    // the long form over the other channels, one launch per K in use: a launch's blocks leave another K's channels alone
    for (int f = 0; f < 2; f++) {
        const ChanList &l = lms_long_lists[3 * f + pos];
        if (!l.n) continue;
        const unsigned Ks = lms_long_Ks[3 * f + pos];
#define QH_LMS_LONG(K) if (Ks & K) hipLaunchKernelGGL(lms_long_kernel<K>, dim3((unsigned)l.n), dim3(64), 0, stream, b, buf_cap, (int)k.n_mid, (const int *)l.dev, \
                                                      (const LmsParam *)lms_prm[f], lms_state[f], lms_long_rows[f])
        QH_LMS_LONG(2); QH_LMS_LONG(4); QH_LMS_LONG(8); QH_LMS_LONG(16); QH_LMS_LONG(32);
#undef QH_LMS_LONG
    }
    if (lists[L_EMNR + pos].n)
        hipLaunchKernelGGL(emnr_kernel, dim3((unsigned)lists[L_EMNR + pos].n), dim3(NT), (size_t)emnr_lds_bytes(), stream, b, buf_cap, k.nblk, lists[L_EMNR + pos].dev,
                           emnr_prm, emnr_chan, emnr_scal, emnr_state, emnr_window, tw4096, emnr_GG, emnr_GGS, emnr_zeta, emnr_zeta_true);
}

// xbandpass (bp1) at position pos, from the rows of cur to those of other -- unless bp1 ended the AM / SAM channels' chain already
void Engine::bp1_at(const ChainCall &k, int pos)
{
    if (lists[L_BP1P + pos].n && !k.direct)
        run_band(k.cur, buf_cap, k.other, buf_cap, nullptr, k.n_mid, fc[FC_BP1], k.P, lists[L_BP1P + pos].dev, lists[L_BP1P + pos].n);
}

// xwcpagc modes 1-4.  Long calls: the level detector in time tiles, everything around it lane-parallel (qh_agc_tiled.hpp).  Short
// calls (the drop-in's blocks), a channel whose attack window moved in mid-stream, and the diagnostic forms: one wavefront per channel.
int Engine::run_agc(ChainCall &k)
{
    const long long n_mid = k.n_mid;
    double2 *cur = k.cur, *other = k.other;
    bool tiled = (wide.agc_form == 0 || wide.agc_form == 3) && n_mid >= kAgcTiledMin;      // (3: diagnostics, the tiles' check counts and repairs nothing)
    int a_max = 0;
    for (int ch = 0; ch < nch && tiled; ch++) {
        ChanCfg &c = cfg[(size_t)ch];
        if (!c.agc_on() || c.w.agc_stale) continue;
        a_max = c.w.agc_abuf > a_max ? c.w.agc_abuf : a_max;
    }
    // the tiles take the channels at the head of each list, the stepping kernel the ones behind them (all of them in a short call)
    const int nt_cur = tiled ? lists[L_AGC_CUR].n - n_agc_cur_stale : 0, nt_other = tiled ? lists[L_AGC_OTHER].n - n_agc_other_stale : 0;
    if (nt_cur + nt_other == 0) tiled = false;
    agc_last_tiled = nt_cur + nt_other;
    for (ChanCfg &c : cfg) if (c.agc_on()) c.w.agc_ran = true;
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
            if (c.agc_on() && c.w.agc_rewindow) rw.push_back(ch);
            if (c.agc_on()) c.w.agc_rewindow = false;
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
    bool no_p1 = !lists[L_BP1P + 1].n && !lists[L_FIX].n && !lists[L_FIX + 1].n && !lists[L_EMNR + 1].n && !lists[L_EMNR + 2].n && !lists[L_AMSQ].n && !wide.meters_on && !k.taps && !eg.kind && !lists[L_AP].n && !lists[L_AP + 1].n &&
                 !ssql_lists.any();
    for (int f = 0; f < 2; f++) for (int p = 1; p < 3; p++) no_p1 = no_p1 && !lms_n(3 * f + p);
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
                               (const double *)bnd, agc_ends_cap * kAgcEndsW, end, agc_ends_cap * kAgcEndsW, L, agc_fin, agc_nfixed, wide.agc_form == 3 ? 1 : 0);
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
        hipLaunchKernelGGL(wide.agc_form == 1 ? wcpagc_seq_kernel : wcpagc_kernel, dim3((unsigned)ns), dim3(64), 0, stream, cur, buf_cap, (int)n_mid,
                           (const int *)(lists[L_AGC_CUR].dev + nt_cur), agc_prm, agc_state, 1.0);
    if (const int ns = lists[L_AGC_OTHER].n - nt_other)
        hipLaunchKernelGGL(wide.agc_form == 1 ? wcpagc_seq_kernel : wcpagc_kernel, dim3((unsigned)ns), dim3(64), 0, stream, other, buf_cap, (int)n_mid,
                           (const int *)(lists[L_AGC_OTHER].dev + nt_other), agc_prm, agc_state, 1.0);
    return QH_OK;
}

// xsender (RXA.c:570): the listed channels' rows behind nbp0 and the S meter, ahead of xamsqcap and bpsnba, narrowed to float pairs
void Engine::run_sender(const ChainCall &k)
{
    if (!k.taps || !tap_lists[0].n) return;
    const long long per = (k.n_mid + NT - 1) / NT;
    hipLaunchKernelGGL(sender_tap_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)tap_lists[0].n), dim3(NT), 0, stream,
                       (const double2 *)k.cur, buf_cap, (int)k.n_mid, (const int *)tap_lists[0].dev, snd_rows, snd_cap);
}

// xgen (RXA.c:565): the listed channels' rows behind xshift and xresample, which have run and moved their state on, are replaced; the
// adc meter, bpsnba's input, nbp0 and everything behind them read the generated signal.  Then the running modes' state moves on.
void Engine::run_gen(const ChainCall &k)
{
    if (!k.gen || !gen_lists[0].n) return;
    const long long per = (k.n_mid + NT - 1) / NT;
    hipLaunchKernelGGL(gen_kernel, dim3((unsigned)(per < 1024 ? per : 1024), (unsigned)gen_lists[0].n), dim3(NT), 0, stream, k.cur, buf_cap, (int)k.n_mid,
                       (const int *)gen_lists[0].dev, (const GenParam *)gen_prm, (const GenState *)gen_state, (const double2 *)gen_ck, (const double *)gen_ctrans);
    hipLaunchKernelGGL(gen_advance_kernel, dim3((unsigned)((gen_lists[0].n + 255) / 256)), dim3(256), 0, stream, (int)k.n_mid, (const int *)gen_lists[0].dev, gen_lists[0].n,
                       (const GenParam *)gen_prm, gen_state);
}

// xsiphon (RXA.c:590): the listed channels' rows behind bp1 at position 1 and the agc meter (cur / other, as the meter reads them), ahead
// of xcbl; a fixed AGC gain that the output matrix has still to apply goes in with the copy (tap_gain)
void Engine::run_siphon(const ChainCall &k)
{
    if (!k.taps || (!tap_lists[1].n && !tap_lists[2].n)) return;
    const long long span = k.n_mid < kSipSize ? k.n_mid : kSipSize;
    const unsigned gx = (unsigned)((span + NT - 1) / NT);
    for (int b = 0; b < 2; b++) {
        const ChanList &l = tap_lists[1 + b];
        if (!l.n) continue;
        hipLaunchKernelGGL(siphon_tap_kernel, dim3(gx, (unsigned)l.n), dim3(NT), 0, stream, (const double2 *)(b ? k.other : k.cur), buf_cap,
                           (int)k.n_mid, dsp_size, (const int *)l.dev, (const double *)tap_gain, sip_ring, (const int *)sip_idx);
        if (dsp_size < kSipSize)
            hipLaunchKernelGGL(siphon_advance_kernel, dim3((unsigned)((l.n + 255) / 256)), dim3(256), 0, stream, (int)k.n_mid, (const int *)l.dev, l.n, sip_idx);
    }
}

// The last call's sender rows to sub-span ss of a display bank with a display per channel, on the device: the bank's stream waits for
// the engine's (qh_ana_feed_f32), and the engine's next call for the bank's append (process_fed) -- events both ways, no host wait.
// Spectrum2 reads element 2i + 1 as I (analyzer.c:1503-1507) and xsender hands it the chain's (I, Q) rows as they are: swap_iq = 1.
int Engine::feed_display(qh_ana *a, int ss)
{
    if (!a) return set_error(QH_ERR_INVALID, "null analyzer");
    if (qh_ana_ndisp(a) != nch || qh_ana_buff_size(a) != dsp_size || qh_ana_device(a) != device)
        return set_error(QH_ERR_INVALID, "the display bank needs a display per channel (%d), buff_size = dsp_size (%d) and the engine's device", nch, dsp_size);
    if (!snd_rows || snd_n <= 0 || tap_lists[0].n != nch) return set_error(QH_ERR_INVALID, "the last call left no sender rows of every channel");
    QH_HIP(hipSetDevice(device));
    if (!disp_fed) QH_HIP(hipEventCreateWithFlags(&disp_fed, hipEventDisableTiming));
    if (int rc = qh_ana_feed_f32(a, ss, snd_rows, snd_cap, (int)snd_n, 1, stream, nullptr)) return rc;
    QH_HIP(hipEventRecord(disp_fed, (hipStream_t)qh_ana_stream(a)));
    disp_fed_pending = true;
    return QH_OK;
}

// A process call of the C ABI: the chain (replayed from its captured launch sequence or not), then the attached display's feed.  The
// feed is host-orchestrated (which frames are complete decides the launches), so it stays outside the captured sequence, and so does
// the wait for the last feed's append, which has read the rows this call overwrites.
int Engine::process_fed(bool replay, const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk)
{
    if (disp_fed_pending) {
        QH_HIP(hipSetDevice(device));
        QH_HIP(hipStreamWaitEvent(stream, disp_fed, 0));
        disp_fed_pending = false;
    }
    const int rc = replay ? process_replayed(d_in, in_stride, d_out, out_stride, nblk) : process(d_in, in_stride, d_out, out_stride, nblk);
    if (rc || !wide.disp || nblk <= 0) return rc;
    return feed_display(wide.disp, wide.disp_ss);
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

// the squelch of the listed channels, in place on the rows that hold them behind bp1 (cur / other)
void Engine::run_ssql(const ChainCall &k)
{
    if (!ssql_prm || !ssql_lists.any()) return;
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
    if (lists[L_BP1].n) fc[FC_BP1].flip();       // the launches of both positions, and of run_am, read the one half
    if (wide.meters_on) {    // agcmeter sits after xwcpagc (RXA.c:589); mode 0's gain multiply is applied below, so its
                        // level reading is taken on the fixed-gain input times g^2 (m_g2)
        if (lists[L_PLAIN].n) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)lists[L_PLAIN].n), dim3(64), 0, stream, k.cur, buf_cap, k.nblk, dsp_size,
                                        m_agc, m_prm, lists[L_PLAIN].dev, (const double *)m_g2);
        if (lists[L_BP1].n) hipLaunchKernelGGL(meter_kernel, dim3((unsigned)lists[L_BP1].n), dim3(64), 0, stream, k.other, buf_cap, k.nblk, dsp_size,
                                      m_agc, m_prm, lists[L_BP1].dev, (const double *)m_g2);
    }
    run_siphon(k);                      // xsiphon (RXA.c:590)
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

int Engine::process_replayed(const double *d_in, long long in_stride, double *d_out, long long out_stride, int nblk)
{
    // the resamplers (the output one; the input one of the rate ratios that are not 1, 2, 4, 8 or 16) keep a host-side phase and their
    // own ping-pong of delay lines per call, event timing records per call: all of them stay on the plain path.  (The input resampler was
    // missing here until a seeded walk through the WDSP names at 144 ksps found it: a sequence captured after a setter replayed the
    // other parity of its delay lines, tests/test_gpu_wdsp_names_fuzz.py.)
    if (rsmpin || rsmpout || wide.timing || nblk <= 0) return process(d_in, in_stride, d_out, out_stride, nblk);
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
        wide.graph_on = false;
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
    wide.graph_on = false;
    return process(d_in, in_stride, d_out, out_stride, nblk);
}

}  // namespace qh

#ifdef QH_AGC_COUNT
extern "C" int qh_dbg_agc_counts(unsigned long long *out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(qh::g_agc_count), 20 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[20] = { 0 }; if (hipMemcpyToSymbol(HIP_SYMBOL(qh::g_agc_count), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif
