// qh_div.hip -- WDSP's diversity combiner DIV (include/quiskhip.h group 10e): xdiv and its setters, wdsp/div.c:31-95,136-187, for
// `ngroups` groups of up to eight phase-coherent receivers, fp64 complex, every group with its own run, nr, output and rotate factors.
//
// The reference, per group: run = 0 copies receiver 0; output != nr copies receiver `output` (nothing where out is that row); output ==
// nr zeroes out and adds, receiver by receiver, the receiver's samples times its complex rotate factor.  No sample looks at another
// one and nothing is kept from call to call, so a call is one launch: the grid runs over tiles of kDivTile samples x groups, a lane
// takes whole complex samples (16-byte loads and stores), issues the loads of a sample's nr rows before it uses the first and keeps the
// running sum in registers -- nr reads and one write per sample.  The sum is the reference's bit for bit: it starts from +0.0, and every
// product, the difference or sum of the two products and the accumulation are rounded on their own (fp contract off).
//
// out laid over a receiver's row (the reference's callers hand out == in[k]): the memset has zeroed that row before the loop reads it,
// and the loop then reads the running sum back at i = k.  The kernel takes a mask of the receivers whose row is the output row and
// gives them the running sum in place of their samples; every sample is loaded and stored by one lane, so nothing else has to be
// ordered.
#include <algorithm>
#include <cmath>
#include <vector>
#include "qh_bank.hpp"

using namespace qh;

namespace {

constexpr int kDivMaxNr = 8;                            // MAX_NR, div.c:29
constexpr int kDivBlock = 256, kDivPerLane = 4, kDivTile = kDivBlock * kDivPerLane;

struct DivParam {
    double ir[kDivMaxNr], qr[kDivMaxNr];
    int nr;                                             // receivers mixed
    int src;                                            // -1: mix; else the receiver copied
    int pad[2];
};
static_assert(sizeof(DivParam) == 144, "the layout the kernel and the upload share");

// U samples of a lane, kDivBlock apart: every load of the NR rows first, then div.c:81-89 in the reference's order of i.
template <int NR, int U, bool TAIL>
__device__ __forceinline__ void div_mix(const double2 *__restrict__ row0, long long rx_stride, double2 *orow, long long j0, int n, const DivParam &p,
                                        unsigned alias)
{
    double2 x[NR][U];
#pragma unroll
    for (int i = 0; i < NR; i++)
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long j = j0 + (long long)u * kDivBlock;
            x[i][u] = (!TAIL || j < n) ? row0[(long long)i * rx_stride + j] : make_double2(0.0, 0.0);
        }
    double2 s[U];
#pragma unroll
    for (int u = 0; u < U; u++) s[u] = make_double2(0.0, 0.0);                  // memset, div.c:81
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < NR; i++) {
            const double ir = p.ir[i], qr = p.qr[i];
            const bool back = (alias >> i) & 1u;                                // this receiver's row is the output row
#pragma unroll
            for (int u = 0; u < U; u++) {
                const double I = back ? s[u].x : x[i][u].x, Q = back ? s[u].y : x[i][u].y;
                const double a = ir * I, b = qr * Q, c = ir * Q, d = qr * I;
                const double re = a - b, im = c + d;
                s[u].x = s[u].x + re;                                           // div.c:87
                s[u].y = s[u].y + im;                                           // div.c:88
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const long long j = j0 + (long long)u * kDivBlock;
        if (!TAIL || j < n) orow[j] = s[u];
    }
}

// A tile of kDivTile samples in batches that keep up to eight 16-byte loads of a lane in flight.
template <int NR, bool TAIL>
__device__ __forceinline__ void div_mix_tile(const double2 *__restrict__ row0, long long rx_stride, double2 *orow, long long t0, int n, const DivParam &p,
                                             unsigned alias)
{
    constexpr int U = NR <= 2 ? 4 : NR <= 4 ? 2 : 1;
#pragma unroll
    for (int b = 0; b < kDivPerLane / U; b++)
        div_mix<NR, U, TAIL>(row0, rx_stride, orow, t0 + (long long)b * U * kDivBlock + threadIdx.x, n, p, alias);
}

template <bool TAIL>
__device__ __forceinline__ void div_tile(const double2 *__restrict__ row0, long long rx_stride, double2 *orow, long long t0, int n, const DivParam &p,
                                         unsigned alias)
{
    if (p.src >= 0) {                                                           // div.c:72-76, :94
        if ((alias >> p.src) & 1u) return;                                      // out is in[output]: nothing to do
        const double2 *__restrict__ irow = row0 + (long long)p.src * rx_stride;
        double2 v[kDivPerLane];
#pragma unroll
        for (int u = 0; u < kDivPerLane; u++) {
            const long long j = t0 + (long long)u * kDivBlock + threadIdx.x;
            v[u] = (!TAIL || j < n) ? irow[j] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < kDivPerLane; u++) {
            const long long j = t0 + (long long)u * kDivBlock + threadIdx.x;
            if (!TAIL || j < n) orow[j] = v[u];
        }
        return;
    }
    switch (p.nr) {                                                             // (uniform over the block)
    case 1: div_mix_tile<1, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    case 2: div_mix_tile<2, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    case 3: div_mix_tile<3, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    case 4: div_mix_tile<4, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    case 5: div_mix_tile<5, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    case 6: div_mix_tile<6, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    case 7: div_mix_tile<7, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    case 8: div_mix_tile<8, TAIL>(row0, rx_stride, orow, t0, n, p, alias); break;
    default: break;
    }
}

// xdiv (div.c:67-95) for every group: block (t, g) makes samples t kDivTile ... of group g.  alias: bit i set where receiver i's row is
// the group's output row.  Offsets in 64 bits: g * group_stride can pass 2^31.
__global__ __launch_bounds__(kDivBlock) void div_kernel(const double2 *__restrict__ in, long long rx_stride, long long group_stride, double2 *out,
                                                        long long out_stride, int n, const DivParam *__restrict__ prm, unsigned alias)
{
    const long long g = blockIdx.y, t0 = (long long)blockIdx.x * kDivTile;
    const DivParam &p = prm[g];
    const double2 *__restrict__ row0 = in + g * group_stride;
    double2 *orow = out + g * out_stride;
    if (t0 + kDivTile <= n) div_tile<false>(row0, rx_stride, orow, t0, n, p, alias);
    else div_tile<true>(row0, rx_stride, orow, t0, n, p, alias);
}

struct DivSettings {
    int run, nr, output;
    double ir[kDivMaxNr], qr[kDivMaxNr];
};

const char *div_refusal(const DivSettings &s)
{
    if (s.nr < 1 || s.nr > kDivMaxNr) return "nr must lie in 1..8 (MAX_NR, div.c:29)";
    if (s.output < 0 || s.output > kDivMaxNr) return "output must lie in 0..8";
    for (int i = 0; i < kDivMaxNr; i++)
        if (!std::isfinite(s.ir[i]) || !std::isfinite(s.qr[i])) return "the rotate factors must be finite";
    return nullptr;
}

// [p, p + len) and [q, q + len) share a byte
inline bool div_meet(long long p, long long q, long long len) { return p < q + len && q < p + len; }

}  // namespace

struct qh_div : Bank {
    std::vector<DivSettings> set;
    std::vector<DivParam> prm;
    DivParam *d_prm = nullptr;
    ~qh_div()
    {
        quiesce();
        (void)hipFree(d_prm);
    }

    static const char *refusal(const DivSettings &s) { return div_refusal(s); }
    void derive(int) {}                                 // (bank_set's restarting setters: DIV keeps nothing from call to call)
    int restart(int, int) { return QH_OK; }

    void apply_light(int g)
    {
        const DivSettings &s = set[g];
        DivParam &p = prm[g];
        std::copy(s.ir, s.ir + kDivMaxNr, p.ir);
        std::copy(s.qr, s.qr + kDivMaxNr, p.qr);
        p.nr = s.nr;
        p.src = !s.run ? 0 : s.output != s.nr ? s.output : -1;                 // div.c:69,72,94
        p.pad[0] = p.pad[1] = 0;
    }

    // host settings -> device, behind everything enqueued so far (the copy is synchronous: the vector may change right after)
    int upload()
    {
        if (!dirty) return QH_OK;
        QH_HIP(hipStreamSynchronize(stream));
        QH_HIP(hipMemcpy(d_prm, prm.data(), (size_t)nch * sizeof(DivParam), hipMemcpyHostToDevice));
        dirty = false;
        return QH_OK;
    }

    // Whether the call reads receiver i of group g
    bool reads(int g, int i) const { return prm[g].src < 0 ? i < prm[g].nr : i == prm[g].src; }

    // The arguments and the settings of a process call on rows `in` / `out` (device or host addresses alike; mtx held).  alias: the
    // receivers whose row is the output row, where the caller has not said (*alias < 0 on entry): bit k for out == in + k rx_stride with
    // out_stride == group_stride.  Any other byte an output row shares with a row the call reads is refused; the output rows are apart
    // from each other because out_stride >= n.
    int check_call(const char *name, const void *in, long long rx_stride, long long group_stride, const void *out, long long out_stride, int n,
                   int *alias) const
    {
        if (n < 0 || (n > 0 && (!in || !out))) return set_error(QH_ERR_INVALID, "%s: bad arguments", name);
        if (rx_stride < n || group_stride < n || out_stride < n) return set_error(QH_ERR_INVALID, "%s: a stride is below n", name);
        for (int g = 0; g < nch; g++)
            if (set[g].run && set[g].output > set[g].nr)
                return set_error(QH_ERR_INVALID, "%s: group %d has output %d above its nr %d (the reference reads a receiver nobody handed it)", name, g,
                                 set[g].output, set[g].nr);
        if (n == 0) return QH_OK;
        const long long a = (long long)reinterpret_cast<uintptr_t>(in), o = (long long)reinterpret_cast<uintptr_t>(out), len = (long long)n * 16;
        const long long rx = rx_stride * 16, gs = group_stride * 16, os = out_stride * 16;
        const bool apart = o + (nch - 1) * os + len <= a || a + (nch - 1) * gs + (kDivMaxNr - 1) * rx + len <= o;   // all of out from all of in
        if (*alias >= 0) {                              // the caller staged the rows and says which receivers were the output row
            if (!apart) return set_error(QH_ERR_INVALID, "%s: the output rows overlap the input rows", name);
            return QH_OK;
        }
        *alias = 0;
        if (apart) return QH_OK;
        int k = -1;
        if (os == gs)
            for (int i = 0; i < kDivMaxNr; i++)
                if (o == a + i * rx) k = i;
        if (k >= 0) *alias = 1 << k;
        // the rows of receiver i ascend with g and lie apart (group_stride >= n), and so do the output rows: one merge walk per receiver
        for (int i = 0; i < kDivMaxNr; i++) {
            for (long long g = 0, h = 0; g < nch && h < nch;) {
                const long long o0 = o + g * os, i0 = a + h * gs + i * rx;
                if (div_meet(o0, i0, len) && reads((int)h, i) && !(i == k && g == h))
                    return set_error(QH_ERR_INVALID, "%s: the output row of group %lld shares bytes with receiver %d of group %lld (an output row may only "
                                     "be exactly one of its own group's rows)", name, g, i, h);
                if (o0 <= i0) g++;
                else h++;
            }
        }
        return QH_OK;
    }

    int launch(const void *d_in, long long rx_stride, long long group_stride, void *d_out, long long out_stride, int n, int alias)
    {
        QH_HIP(hipSetDevice(device));
        if (int rc = upload()) return rc;
        hipLaunchKernelGGL(div_kernel, dim3((unsigned)(((long long)n + kDivTile - 1) / kDivTile), (unsigned)nch), dim3(kDivBlock), 0, stream,
                           static_cast<const double2 *>(d_in), rx_stride, group_stride, static_cast<double2 *>(d_out), out_stride, n, d_prm, (unsigned)alias);
        QH_HIP(hipGetLastError());
        return QH_OK;
    }
};

int qh::div_process_staged(qh_div *h, const void *d_in, long long rx_stride, long long group_stride, void *d_out, long long out_stride, int n,
                           unsigned alias)
{
    if (!h || alias > 0xffu) return set_error(QH_ERR_INVALID, "qh_div_process: bad arguments");
    std::lock_guard<std::mutex> lk(h->mtx);
    int al = (int)alias;
    if (int rc = h->check_call("qh_div_process", d_in, rx_stride, group_stride, d_out, out_stride, n, &al)) return rc;
    if (n == 0) return QH_OK;
    return h->launch(d_in, rx_stride, group_stride, d_out, out_stride, n, al);
}

extern "C" {

qh_div *qh_div_create(int device, int ngroups, int run, int nr, void *stream)
{
    DivSettings s0{};                                   // output 0 and the rotate factors 0: malloc0, div.c:34-43
    s0.run = run;
    s0.nr = nr;
    if (ngroups <= 0 || ngroups > 65535) { set_error(QH_ERR_INVALID, "qh_div_create: bad arguments"); return nullptr; }
    if (const char *why = div_refusal(s0)) { set_error(QH_ERR_INVALID, "qh_div_create: %s", why); return nullptr; }
    qh_div *h = new qh_div();
    h->nch = ngroups;
    if (bank_open(h, device, stream, "qh_div_create") != QH_OK) { delete h; return nullptr; }
    h->set.assign((size_t)ngroups, s0);
    h->prm.assign((size_t)ngroups, DivParam{});
    for (int g = 0; g < ngroups; g++) h->apply_light(g);
    if (dev_alloc(&h->d_prm, (size_t)ngroups) != hipSuccess) {
        set_error(QH_ERR_HIP, "qh_div_create: hipMalloc failed");
        delete h;
        return nullptr;
    }
    return h;
}

void qh_div_destroy(qh_div *h) { delete h; }

int qh_div_set_run(qh_div *h, int g, int run) { return bank_set(h, g, "qh_div_set_run", false, [=](DivSettings &s) { s.run = run; }); }
int qh_div_set_nr(qh_div *h, int g, int nr) { return bank_set(h, g, "qh_div_set_nr", false, [=](DivSettings &s) { s.nr = nr; }); }
int qh_div_set_output(qh_div *h, int g, int output) { return bank_set(h, g, "qh_div_set_output", false, [=](DivSettings &s) { s.output = output; }); }

int qh_div_set_rotate(qh_div *h, int g, int nr, const double *Irotate, const double *Qrotate)
{
    if (nr < 0 || nr > kDivMaxNr || !Irotate || !Qrotate)
        return set_error(QH_ERR_INVALID, "qh_div_set_rotate: nr must lie in 0..8 and the arrays must be there (the reference copies nr values into arrays of 8)");
    return bank_set(h, g, "qh_div_set_rotate", false, [=](DivSettings &s) {
        std::copy(Irotate, Irotate + nr, s.ir);
        std::copy(Qrotate, Qrotate + nr, s.qr);
    });
}

int qh_div_get(qh_div *h, int g, int *run, int *nr, int *output, double *Irotate8, double *Qrotate8)
{
    if (!h || g < 0 || g >= h->nch) return set_error(QH_ERR_INVALID, "qh_div_get: bad arguments");
    std::lock_guard<std::mutex> lk(h->mtx);
    const DivSettings &s = h->set[g];
    if (run) *run = s.run;
    if (nr) *nr = s.nr;
    if (output) *output = s.output;
    if (Irotate8) std::copy(s.ir, s.ir + kDivMaxNr, Irotate8);
    if (Qrotate8) std::copy(s.qr, s.qr + kDivMaxNr, Qrotate8);
    return QH_OK;
}

int qh_div_process(qh_div *h, const void *d_in, long long rx_stride, long long group_stride, void *d_out, long long out_stride, int n)
{
    if (!h) return set_error(QH_ERR_INVALID, "qh_div_process: bad arguments");
    std::lock_guard<std::mutex> lk(h->mtx);
    int alias = -1;
    if (int rc = h->check_call("qh_div_process", d_in, rx_stride, group_stride, d_out, out_stride, n, &alias)) return rc;
    if (n == 0) return QH_OK;
    return h->launch(d_in, rx_stride, group_stride, d_out, out_stride, n, alias);
}

// Host rows: the rows the call reads go to device rows [ngroups][rows][n], the output rows come back; an output row laid over a
// receiver's row is laid over it on the device too.  Returns when the output is in h_out.
int qh_div_process_host(qh_div *h, const void *h_in, long long rx_stride, long long group_stride, void *h_out, long long out_stride, int n)
{
    const char *name = "qh_div_process_host";
    if (!h) return set_error(QH_ERR_INVALID, "%s: bad arguments", name);
    std::lock_guard<std::mutex> lk(h->mtx);
    int alias = -1;
    if (int rc = h->check_call(name, h_in, rx_stride, group_stride, h_out, out_stride, n, &alias)) return rc;
    if (n == 0) return QH_OK;
    QH_HIP(hipSetDevice(h->device));
    int k = -1, rows = 1;
    for (int i = 0; i < kDivMaxNr; i++)
        if ((alias >> i) & 1) k = i;
    for (int g = 0; g < h->nch; g++) rows = std::max(rows, h->prm[g].src < 0 ? h->prm[g].nr : h->prm[g].src + 1);
    rows = std::max(rows, k + 1);
    const size_t ng = (size_t)h->nch, row = (size_t)n * 16;
    double2 *d = nullptr, *o = nullptr;
    QH_HIP(hipMalloc((void **)&d, ng * (size_t)rows * row));
    if (k < 0 && hipMalloc((void **)&o, ng * row) != hipSuccess) { (void)hipFree(d); return set_error(QH_ERR_HIP, "%s: hipMalloc failed", name); }
    const long long d_gs = (long long)rows * n;
    double2 *d_out = k < 0 ? o : d + (size_t)k * (size_t)n;
    const long long d_os = k < 0 ? n : d_gs;
    int rc = QH_OK;
    for (int g = 0; g < h->nch && rc == QH_OK; g++) {
        const DivParam &p = h->prm[g];
        const int r0 = p.src < 0 ? 0 : p.src, cnt = p.src < 0 ? p.nr : 1;
        const char *src = static_cast<const char *>(h_in) + ((size_t)g * (size_t)group_stride + (size_t)r0 * (size_t)rx_stride) * 16;
        if (hipMemcpy2DAsync(d + (size_t)g * (size_t)d_gs + (size_t)r0 * (size_t)n, row, src, (size_t)rx_stride * 16, row, (size_t)cnt, hipMemcpyHostToDevice,
                             h->stream) != hipSuccess)
            rc = set_error(QH_ERR_HIP, "%s: upload failed", name);
    }
    if (rc == QH_OK) rc = h->launch(d, n, d_gs, d_out, d_os, n, alias);
    if (rc == QH_OK && hipMemcpy2DAsync(h_out, (size_t)out_stride * 16, d_out, (size_t)d_os * 16, row, ng, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = set_error(QH_ERR_HIP, "%s: download failed", name);
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == QH_OK) rc = set_error(QH_ERR_HIP, "%s: synchronize failed", name);
    (void)hipFree(d); (void)hipFree(o);
    return rc;
}

int qh_div_synchronize(qh_div *h) { return bank_synchronize(h, "qh_div_synchronize"); }

}  // extern "C"
