"""The AM, SAM and FM detectors of the RXA chain -- xamd (wdsp/amd.c:115-239) and xfmd (wdsp/fmd.c:144-188) with the filters behind
them -- as sample loops written once over a number type, run in long double (`want`) and in float64 on a float64 overlap-save model of
the linear chain ahead of them (`model`), and the per-sample bound the engine's detector kernels are held to.  numpy only; built on
tests/rxa_linear_ref.py (the oscillator's contract, the taps, conv_ld, upsample, os_filter64, panel).

    d[m]    = nbp0's output ahead of gain and panel             rxa_linear_ref: rotation, resampler, fir_bandpass, in long double / float64
    AM      : env = |d|, the fade leveller, bp1, fixed gain, panel
    SAM     : the loop (zeta 1, omega_N 250) on d, the mix with the phase each sample saw, the all-pass chains of SAM-L / SAM-U,
              the fade leveller, bp1, fixed gain, panel
    FM      : the loop (zeta 1, omega_N 20000) on d, dc removal and `again`, de-emphasis, audio filter, CTCSS notch (I only), panel
              (SetRXAMode switches the AGC off in FM, RXA.c:775: no fixed gain there)

Every case primes the chain for PRIME blocks in USB mode with the detector's own passband already set, then SetRXAMode switches the
detector in: the linear part stays time-invariant, the detector meets a strong carrier from its first sample, and its loop's pull-in is
a smooth function of the input (atan2 on the round-off that fills an empty filter is chaotic in the reference too).  The carrier's
phase is chosen so that the loop starts near the middle of the detector's range.  bp1, the de-emphasis and the audio filter start from
empty delay lines at the switch (RXAbp1Set flushes bp1 when it comes on; xfmd never ran).  The shift frequencies are whole multiples of
2^-64 turns a sample at 192 kHz, so the oscillator's step is exact and has no term in the bound.

Bound, per output sample behind the switch and per part:

    |got - want| <= 16 E                        while the loop has stepped in order since the switch
    |got - want| <= 16 E + T                    from the first call on in which tiles are accepted by comparing states

E is the largest per-part |model - want| behind the switch; 16 is rxa_linear_ref.MARGIN.  A time-tiled call (FM: more than 4 tiles of
256 samples; SAM: from 32768 samples on) starts every tile but the first few from a warmed-up guess and accepts it when phase (in
turns), loop filter output and omega agree with the previous tile's end to TILE_TOL = 1e-12 (qh_tiled.hpp pll_state_differs): T is the
largest deviation of the CHAIN'S OUTPUT over every sign pattern of such a difference at a tile boundary of the case, from the
long-double loop alone, doubled (a tile inherits what its predecessor was accepted with, and the loop contracts).  The loop's response
to 1e-12 is linear to 1e-24, so the largest over the eight sign patterns is the sum of the magnitudes of the three single responses.
The loop's own state is exact again a tile later (it contracts by e^-100 over an FM tile, e^-21 over a SAM tile), but the filters behind
it (2 x 2047 taps in FM, 2047 in SAM) and the notch keep the deviating samples: T stays in the bound for the calls that follow.
"""
import collections
import functools

import numpy as np

import rxa_linear_ref as R
from rxa_linear_ref import CLD, LD, MARGIN, assert_inside, rms, worst_sample  # noqa: F401  (the tests take them from here)

TWOPI = 6.2831853071795864                      # wdsp/comm.h:147, as xamd and xfmd wrap the phase with it
IN_RATE, DSP_RATE, DSP_SIZE, PER_IN, NC = 192000, 48000, 256, 1024, 2048
USB, FM, AM, SAM = 1, 5, 6, 10
PRIME = 12
SHIFTS = (9000.0, -12000.0, 10500.0)            # 3/64, -1/16 and 7/128 of 192 kHz: exact in 2^-64 turns
FM_TILE, FM_EXACT_TILES = 256, 4                # qh_engine.hpp kFmTile; kFmWarm = 3 tiles: tile 4 is the first to start from a guess
SAM_TILE, SAM_TILED_MIN, SAM_EXACT_TILES = 4096, 32768, 3   # kSamTile, kSamTiledMin; kSamWarm = 2 tiles
TILE_TOL = 1e-12                                # pll_state_differs
AGC_DB = 6.0
BANDS = {"usb": (300.0, 3000.0), "am": (-4000.0, 4000.0), "sam": (-4000.0, 4000.0), "fm": (-8000.0, 8000.0)}
FM_SCHEDULE = (1, 1, 3, 4, 5, 16, 66, 1, 20)
AM_SCHEDULE = (1, 1, 15, 16, 17, 66, 1)
SAM_SCHEDULE = (1, 2, 40, 132, 1, 130)
SAM_COLD_SCHEDULE = (132, 1)
NBLOCKS = {"usb": 117, "am": 117, "fm": 117, "sam": 306}        # blocks behind the switch that a channel's reference covers


def nblocks(kind, idx):
    return 133 if kind == "sam" and idx >= 3 else NBLOCKS[kind]     # (the cold SAM channels: one long call and a block)

# One channel: its kind, its ordinal among the channels of that kind (which picks shift, carrier and noise), and the detector's settings.
Chan = collections.namedtuple("Chan", "kind idx levelfade sbmode deviation ctcss_run ctcss_freq nc_de nc_aud")


def chan(kind, idx=0, levelfade=1, sbmode=0, deviation=5000.0, ctcss_run=1, ctcss_freq=254.1, nc_de=NC, nc_aud=NC):
    return Chan(kind, idx, levelfade, sbmode, deviation, ctcss_run, ctcss_freq, nc_de, nc_aud)


# ---------------------------------------------------------------------------------------------------------------------------
# the input and the linear chain ahead of the detector
# ---------------------------------------------------------------------------------------------------------------------------
# SAM channels 3 to 5 are the cold case's: so far off centre that the loop slips cycles through most of the first call behind the switch
# (the pull-in time grows with the square of the offset), and tiles that start from a guess meanwhile fail their check
CARRIER = {"fm": (1500.0, -700.0, 300.0), "am": (0.0, 40.0, -25.0), "sam": (35.0, -12.0, 20.0, 1800.0, -1700.0, 1750.0), "usb": (0.0, 0.0, 0.0)}


def _phase(idx, n):
    step = np.full(n, R.nco_step(SHIFTS[idx % 3], IN_RATE), dtype=np.uint64)
    phase = np.zeros(n, dtype=np.uint64)
    np.cumsum(step[:-1], out=phase[1:])
    return phase


def group_delay_in():
    """The delay of resampler and nbp0 in input samples (both are linear-phase): where the carrier's phase at the switch comes from."""
    h, L, M = R.resampler(IN_RATE, DSP_RATE)
    return (h.size - 1) / 2.0 / L + (NC - 1) / 2.0 * (IN_RATE // DSP_RATE)


@functools.lru_cache(maxsize=None)
def make_input(kind, idx):
    """A carrier of 0.5 that never stops, complex Gaussian noise 80 dB under it, where it lands BEHIND the oscillator.  FM: a 1 kHz tone
    at 3 kHz deviation on a carrier up to 1.5 kHz off centre.  AM / SAM: a two-tone envelope (700 and 1900 Hz), SAM's carrier 12 to
    35 Hz off centre.  USB: tones at 1 and 2.2 kHz.  The carrier passes through phase zero where the detector's first sample is made."""
    n = (PRIME + nblocks(kind, idx)) * PER_IN
    t = np.arange(n, dtype=np.float64) - (PRIME * PER_IN - group_delay_in())        # zero where the detector's first sample is centred
    fc = CARRIER[kind][idx % len(CARRIER[kind])]
    ph = (fc / IN_RATE * t) % 1.0
    if kind == "fm":
        s = 0.5 * np.exp(2j * np.pi * (ph + 3.0 * (1.0 - np.cos(2 * np.pi * ((1000.0 / IN_RATE * t) % 1.0))) / (2 * np.pi)))     # 3 kHz / 1 kHz = 3 rad; no deviation at t = 0
    elif kind == "usb":
        s = 0.4 * np.exp(-2j * np.pi * ((1000.0 / IN_RATE * t) % 1.0)) + 0.2 * np.exp(-2j * np.pi * ((2200.0 / IN_RATE * t) % 1.0))
    else:
        env = 1.0 + 0.4 * np.cos(2 * np.pi * ((700.0 / IN_RATE * t) % 1.0)) + 0.3 * np.cos(2 * np.pi * ((1900.0 / IN_RATE * t) % 1.0) + idx)
        s = 0.5 * env * np.exp(2j * np.pi * ph)
    rng = np.random.default_rng(7000 + 101 * idx + {"usb": 0, "am": 1, "sam": 2, "fm": 3}[kind])
    back = np.conj(R.rotation(_phase(idx, n))).astype(np.complex128)
    x = s * back + 3.5e-5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x.setflags(write=False)
    return x


def _front_case(kind):
    return R.case("detector front " + kind, band=BANDS[kind], kind="clean", schedule="plain")


@functools.lru_cache(maxsize=None)
def front(kind, idx):
    """nbp0's output ahead of gain and panel over the whole stream: (long double, float64 model)."""
    R.require_long_double()
    x = make_input(kind, idx)
    rot = R.rotation(_phase(idx, x.size))
    y, y64 = x.astype(CLD) * rot, x * rot.astype(np.complex128)
    for h, L, M, _ in R.stages(_front_case(kind), 0):
        y = R.conv_ld(R.upsample(y, L), h)[::M]
        y64 = R.os_filter64(R.upsample(y64, L), h)[::M]
    return y, y64


# ---------------------------------------------------------------------------------------------------------------------------
# the sample loops, written once over the number type T
# ---------------------------------------------------------------------------------------------------------------------------
def _ctype(T):
    return CLD if T is LD else np.complex128


def pll_params(omega_n, fmin, fmax, zeta=1.0, rate=float(DSP_RATE)):
    """calc_fmd (fmd.c:29-40) / create_amd (amd.c:72-90): (g1, g2, omega_min, omega_max), in doubles as the reference computes them."""
    g1 = 1.0 - np.exp(-2.0 * omega_n * zeta / rate)
    g2 = -g1 + 2.0 * (1 - np.exp(-omega_n * zeta / rate) * np.cos(omega_n / rate * np.sqrt(1.0 - zeta * zeta)))
    return float(g1), float(g2), TWOPI * fmin / rate, TWOPI * fmax / rate


FM_PLL = pll_params(20000.0, -8000.0, 8000.0)   # RXA.c:198-202
SAM_PLL = pll_params(250.0, -2000.0, 2000.0)    # RXA.c:183-186


def pll_loop(d, prm, T, state=None, keep=()):
    """The loop of xfmd (fmd.c:151-168) and of xamd's SAM branch (amd.c:150-156, 214-230; corr is the same sum of products).
    Returns (fil_out [n], the phase each sample saw [n], {index: (phs, fil_out, omega) ahead of that sample} for the indices in keep)."""
    re, im = np.ascontiguousarray(d.real, dtype=T), np.ascontiguousarray(d.imag, dtype=T)
    g1, g2, omin, omax = (T(v) for v in prm)
    twopi, zero, one = T(TWOPI), T(0), T(1)
    phs, fil, om = state if state is not None else (zero, zero, zero)
    n = re.size
    out_f, out_p, kept = np.empty(n, dtype=T), np.empty(n, dtype=T), {}
    keep = set(keep)
    cos, sin, atan2 = np.cos, np.sin, np.arctan2
    for i in range(n):
        if i in keep:
            kept[i] = (phs, fil, om)
        out_p[i] = phs
        c, s = cos(phs), sin(phs)
        a, b = re[i], im[i]
        c0 = +a * c + b * s
        c1 = -a * s + b * c
        if c0 == zero and c1 == zero:
            c0 = one
        det = atan2(c1, c0)
        del_out = fil
        om = om + g2 * det
        if om < omin:
            om = omin
        if om > omax:
            om = omax
        fil = g1 * det + om
        phs = phs + del_out
        while phs >= twopi:
            phs = phs - twopi
        while phs < zero:
            phs = phs + twopi
        out_f[i] = fil
    return out_f, out_p, kept


def fm_dc(fil, deviation, T, lose=None):
    """fmd.c:169-171: audio = again (fil_out - fmdc).  lose: (index, weight) takes weight onem_mtau fil[index] out of the carried average
    behind that sample -- a planted fault."""
    mtau = T(float(np.exp(-1.0 / (DSP_RATE * 0.02))))
    onem = T(1.0 - float(mtau))
    again = T(DSP_RATE / (deviation * TWOPI))
    dc, out = T(0), np.empty(fil.size, dtype=T)
    for i in range(fil.size):
        dc = mtau * dc + onem * fil[i]
        out[i] = again * (fil[i] - dc)
        if lose is not None and i == lose:
            dc = dc - onem * fil[i]
    return out


def snotch_params(freq, rate=DSP_RATE, bw=0.0002):
    """calc_snotch, iir.c:35-49 (bw: fmd.c:47)."""
    csn = np.cos(TWOPI * (freq / float(rate)))
    qr = 1.0 - 3.0 * bw
    qk = (1.0 - 2.0 * qr * csn + qr * qr) / (2.0 * (1.0 - csn))
    return float(qk), float(-2.0 * qk * csn), float(qk), float(2.0 * qr * csn), float(-qr * qr)


def snotch(x, prm, T, late=None):
    """xsnotch, iir.c:76-95, on a real sequence.  late: at that index the state handed on is the one of a sample earlier (x1, y1 are not
    moved up for one step) -- a planted fault."""
    a0, a1, a2, b1, b2 = (T(v) for v in prm)
    x1 = x2 = y1 = y2 = T(0)
    out = np.empty(x.size, dtype=T)
    for i in range(x.size):
        x0 = x[i]
        y0 = a0 * x0 + a1 * x1 + a2 * x2 + b1 * y1 + b2 * y2
        out[i] = y0
        if late is not None and i == late:
            continue
        y2, y1, x2, x1 = y1, y0, x1, x0
    return out


AMD_C0 = (-0.328201924180698, -0.744171491539427, -0.923022915444215, -0.978490468768238, -0.994128272402075, -0.998458978159551,
          -0.999790306259206)
AMD_C1 = (-0.0991227952747244, -0.565619728761389, -0.857467122550052, -0.959123933111275, -0.988739372718090, -0.996959189310611,
          -0.999282492800792)


def allpass(rows, T):
    """The four all-pass chains of amd.c:160-184 over rows = (ai delayed by one, bi, bq delayed by one, aq): seven stages of
    y[n] = c (x[n] - y[n - 2]) + x[n - 2], c from c0 for the delayed rows and from c1 for the others.  Even and odd samples never meet,
    so the eight sequences step side by side."""
    x = np.stack(rows).astype(T)
    n = x.shape[1]
    m = (n + 1) // 2
    xe = np.zeros((8, m + 1), dtype=T)                          # column 0: the zero ahead of the stream
    xe[0::2, 1:1 + (n + 1) // 2] = x[:, 0::2]
    xe[1::2, 1:1 + n // 2] = x[:, 1::2]
    for c0, c1 in zip(AMD_C0, AMD_C1):
        cv = np.repeat(np.array([c0, c1, c0, c1], dtype=T), 2)
        y = np.zeros_like(xe)
        prev = y[:, 0].copy()
        for k in range(1, m + 1):
            prev = cv * (xe[:, k] - prev) + xe[:, k - 1]
            y[:, k] = prev
        xe = y
    out = np.empty((4, n), dtype=T)
    out[:, 0::2] = xe[0::2, 1:1 + (n + 1) // 2]
    out[:, 1::2] = xe[1::2, 1:1 + n // 2]
    return out


def sam_audio(d, phs, sbmode, T):
    """amd.c:150-205: (audio, corr[0]) from the detector's input and the phase each sample saw."""
    I, Q = np.ascontiguousarray(d.real, dtype=T), np.ascontiguousarray(d.imag, dtype=T)
    c, s = np.cos(phs), np.sin(phs)
    ai, bi, aq, bq = I * c, I * s, Q * c, Q * s
    corr0 = +ai + bq
    if sbmode == 0:
        return corr0, corr0
    zero = np.zeros(1, dtype=T)
    ai_ps, bi_ps, bq_ps, aq_ps = allpass((np.concatenate([zero, ai[:-1]]), bi, np.concatenate([zero, bq[:-1]]), aq), T)
    if sbmode == 1:
        return (ai_ps - bi_ps) + (aq_ps + bq_ps), corr0
    return (ai_ps + bi_ps) - (aq_ps - bq_ps), corr0


def fade_leveller(audio, insert, T, lose=None):
    """amd.c:136-142 / 207-212: dc follows the audio with tauR = 0.02 s, dc_insert follows `insert` (AM: the envelope; SAM: corr[0]) with
    tauI = 1.4 s.  lose: behind that index the slow average has lost that sample's weight -- a planted fault."""
    mR = T(float(np.exp(-1.0 / (DSP_RATE * 0.02))))
    oR = T(1.0 - float(mR))
    mI = T(float(np.exp(-1.0 / (DSP_RATE * 1.4))))
    oI = T(1.0 - float(mI))
    dc = ins = T(0)
    out = np.empty(audio.size, dtype=T)
    for i in range(audio.size):
        dc = mR * dc + oR * audio[i]
        ins = mI * ins + oI * insert[i]
        out[i] = audio[i] + (ins - dc)
        if lose is not None and i == lose:
            ins = ins - oI * insert[i]
    return out


def conv(x, h, T):
    return R.conv_ld(x, h) if T is LD else R.os_filter64(x, h)


@functools.lru_cache(maxsize=None)
def bp1_taps():
    return R.band_taps(NC, -4000.0, 4000.0, DSP_RATE, 1, 2.0)       # bandpass.c:302 at the gain RXAbp1Check sets for AM / SAM


@functools.lru_cache(maxsize=None)
def fm_taps(nc_de, nc_aud):
    import rxa_fm_filters_ref as FF                                 # fc_impulse restated and pinned by tests/test_fm_filters_ref.py
    scale = 2.0 * DSP_SIZE                                          # fircore's transform pair is unnormalised: the designs carry 1 / (2 size)
    return (FF.de_impulse(nc_de, 300.0, 3000.0, DSP_RATE, DSP_SIZE) * scale, FF.aud_impulse(nc_aud, 300.0, 3000.0, DSP_RATE, DSP_SIZE) * scale)


def _pack(audio, T):
    z = np.empty(audio.size, dtype=_ctype(T))
    z.real, z.imag = audio, audio
    return z


# ---------------------------------------------------------------------------------------------------------------------------
# the chains behind the switch
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loop_of(kind, idx, wide):
    """The loop of channel (kind, idx) behind the switch in long double (wide) or on the model in float64: (fil_out, phases, the states
    ahead of every DSP block: calls and tiles start there)."""
    T = LD if wide else np.float64
    d = front(kind, idx)[0 if wide else 1][PRIME * DSP_SIZE:]
    return pll_loop(d, FM_PLL if kind == "fm" else SAM_PLL, T, keep=range(0, d.size, DSP_SIZE) if wide else ())


def fm_tail(audio, ch, T, late=None):
    """xfmd behind the loop and dc removal (fmd.c:173-178) and the panel: de-emphasis, audio filter, CTCSS notch on I."""
    de, aud = fm_taps(ch.nc_de, ch.nc_aud)
    y = conv(conv(_pack(audio, T), de, T), aud, T)
    det = y.copy()
    if ch.ctcss_run:
        det.real = snotch(np.ascontiguousarray(y.real), snotch_params(ch.ctcss_freq), T, late)
    return det, R.panel(det, 0.0)


def am_tail(det, T):
    return R.panel(conv(det, bp1_taps(), T), AGC_DB)


def chain(ch, d, T, loop=None, fault=None):
    """(the detector's own output, the chain's output) of channel ch on the detector input d, in T.  loop: pll_loop's result on d when it is
    at hand.  fault: (name, index, the loop's true state ahead of that index or None) plants one."""
    fname, fidx, fstate = fault if fault else (None, None, None)
    if ch.kind == "usb":
        return d, R.panel(d, AGC_DB)
    if ch.kind == "fm":
        fil = (loop or pll_loop(d, FM_PLL, T))[0]
        if fname == "omega":                        # one tile started 1e-9 off in omega
            st = (T(fstate[0]), T(fstate[1]), T(fstate[2]) + T(1e-9))
            fil = fil.copy()
            fil[fidx:fidx + FM_TILE] = pll_loop(d[fidx:fidx + FM_TILE], FM_PLL, T, state=st)[0]
        audio = fm_dc(fil, ch.deviation, T, lose=fidx if fname == "dc" else None)
        return fm_tail(audio, ch, T, late=fidx if fname == "notch" else None)
    if ch.kind == "am":
        env = np.sqrt(d.real * d.real + d.imag * d.imag).astype(T)
        audio, insert = env, env
    else:
        audio, insert = sam_audio(d, (loop or pll_loop(d, SAM_PLL, T))[1], ch.sbmode, T)
    if ch.levelfade:
        audio = fade_leveller(audio, insert, T, lose=fidx if fname == "leveller" else None)
    det = _pack(audio, T)
    return det, am_tail(det, T)


def detector(ch, wide, fault=None):
    """chain() of a channel's own stream behind the switch, in long double (wide) or as the float64 model.  fault: (name, index)."""
    d = front(ch.kind, ch.idx)[0 if wide else 1][PRIME * DSP_SIZE:]
    loop = loop_of(ch.kind, ch.idx, wide) if ch.kind in ("fm", "sam") else None
    if fault:
        fault = (fault[0], fault[1], loop_of("fm", ch.idx, True)[2].get(fault[1]) if fault[0] == "omega" else None)
    return chain(ch, d, LD if wide else np.float64, loop, fault)


# ---------------------------------------------------------------------------------------------------------------------------
# T: what a tile accepted at TILE_TOL can do to the chain's output
# ---------------------------------------------------------------------------------------------------------------------------
def _linear_tail64(ch, ddet, dins):
    """The chain behind the loop applied to a DEVIATION of the detector's output (everything there is linear), in float64 from rest."""
    T = np.float64
    if ch.kind == "fm":
        de, aud = fm_taps(ch.nc_de, ch.nc_aud)
        y = np.convolve(np.convolve(fm_dc(ddet, ch.deviation, T) * (1 + 1j), de), aud)[:ddet.size]
        yn = snotch(np.ascontiguousarray(y.real), snotch_params(ch.ctcss_freq), T) if ch.ctcss_run else y.real
        return 4.0 * np.maximum(np.maximum(np.abs(y.real), np.abs(yn)), np.abs(y.imag))
    a = fade_leveller(ddet, dins, T) if ch.levelfade else ddet
    y = np.convolve(a * (1 + 1j), bp1_taps())[:a.size]
    return 4.0 * 10.0 ** (AGC_DB / 20.0) * np.maximum(np.abs(y.real), np.abs(y.imag))


@functools.lru_cache(maxsize=None)
def tile_term(ch, boundaries):
    """T of a channel: at each of `boundaries` (indices behind the switch where a tile starts from a guess) the long-double loop is
    started from its true state moved by TILE_TOL in the phase (turns), in fil_out and in omega, one at a time; each deviation of the
    loop is carried through the chain; the magnitudes are added (the largest over the sign patterns) and the whole is doubled."""
    if ch.kind not in ("fm", "sam") or not boundaries:
        return 0.0
    fm = ch.kind == "fm"
    fil, phs, kept = loop_of(ch.kind, ch.idx, True)
    d = front(ch.kind, ch.idx)[0][PRIME * DSP_SIZE:]
    win, tail = (512, 8192) if fm else (16384, 8192)
    worst = 0.0
    for b in boundaries:
        st = kept[b]
        seg = d[b:b + win]
        total = np.zeros(min(win + tail, fil.size - b))
        if not fm:                                  # (from rest in the all-pass chains on both sides: the difference is what counts)
            a1, c1 = sam_audio(seg, phs[b:b + seg.size], ch.sbmode, LD)
        for k, step in enumerate((LD(TWOPI) * LD(TILE_TOL), LD(TILE_TOL), LD(TILE_TOL))):
            moved = tuple(v + step if j == k else v for j, v in enumerate(st))
            f2, p2, _ = pll_loop(seg, FM_PLL if fm else SAM_PLL, LD, state=moved)
            if fm:
                ddet, dins = (f2 - fil[b:b + seg.size]).astype(np.float64), None
            else:
                a2, c2 = sam_audio(seg, p2, ch.sbmode, LD)
                ddet, dins = (a2 - a1).astype(np.float64), (c2 - c1).astype(np.float64)
            pad = total.size - ddet.size
            ddet = np.concatenate([ddet, np.zeros(pad)])
            dins = np.concatenate([dins, np.zeros(pad)]) if dins is not None else None
            total += _linear_tail64(ch, ddet, dins)
        worst = max(worst, float(total.max()))
    return 2.0 * worst


def tiled_calls(kind, schedule):
    """[(first output index behind the switch, outputs, tiled?)] per call."""
    out, m = [], 0
    for nb in schedule:
        n = nb * DSP_SIZE
        tiled = (kind == "fm" and n > FM_EXACT_TILES * FM_TILE) or (kind == "sam" and n >= SAM_TILED_MIN)
        out.append((m, n, tiled))
        m += n
    return out


def guess_boundaries(kind, schedule):
    """The first tile of every tiled call that starts from a guess."""
    tile, exact = (FM_TILE, FM_EXACT_TILES) if kind == "fm" else (SAM_TILE, SAM_EXACT_TILES)
    return tuple(m + exact * tile for m, n, tiled in tiled_calls(kind, schedule) if tiled and n > exact * tile)


# ---------------------------------------------------------------------------------------------------------------------------
# the records
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def channel_ref(ch):
    """A channel's reference over the NBLOCKS of its kind: want, the detector's own output, E of both."""
    det_w, want = detector(ch, True)
    det_m, model = detector(ch, False)

    def worst(a, b):
        return float(max(np.max(np.abs(a.real - b.real)), np.max(np.abs(a.imag - b.imag))))
    return {"want": want, "det": det_w, "model": model, "E": worst(model, want), "E_det": worst(det_m, det_w)}


def channel_bound(ch, schedule):
    """(E, T, the per-sample bound) of a channel over a schedule: E over the schedule's samples, T from its first tiled call on."""
    r = channel_ref(ch)
    n = sum(schedule) * DSP_SIZE
    want, model = r["want"][:n], r["model"][:n]
    E = float(max(np.max(np.abs(model.real - want.real)), np.max(np.abs(model.imag - want.imag))))
    T = tile_term(ch, guess_boundaries(ch.kind, schedule))
    b = np.full(n, MARGIN * E)
    first = [m for m, _, tiled in tiled_calls(ch.kind, schedule) if tiled]
    if first and T:
        b[first[0]:] += T
    return E, T, b


def case_ref(chans, schedule):
    """The record of an engine's run: x [nch, n_in] (prime and all), want [nch, m] behind the switch, E, T, rms per channel, the packed
    bound, the call sizes in blocks."""
    n_in, m = (PRIME + sum(schedule)) * PER_IN, sum(schedule) * DSP_SIZE
    E, T, b = zip(*(channel_bound(ch, schedule) for ch in chans))
    want = np.stack([channel_ref(ch)["want"][:m] for ch in chans])
    bound = np.stack(b)
    return {"x": np.stack([make_input(ch.kind, ch.idx)[:n_in] for ch in chans]), "want": want, "E": list(E), "T": list(T),
            "rms": [rms(w) for w in want], "bound": bound + 1j * bound, "blocks": tuple(schedule)}


def seg_groups(count, n_mid):
    """Engine::seg_groups."""
    G = 256 // count if count > 0 else 1
    while G > 1 and n_mid // (64 * 16 * G) < 8:
        G -= 1
    return max(1, min(G, 8))


def detector_seams(chans, schedule):
    """Output indices behind the switch where FM tiles (256), SAM tiles (4096, in tiled calls), the segments of the scans (16 G of them over
    the call's batches of 64, G as Engine::seg_groups over the channels of the kind) and the calls start: (seams, calls)."""
    kinds = [ch.kind for ch in chans]
    seams, calls, m = [], [], 0
    for nb in schedule:
        n = nb * DSP_SIZE
        calls.append(m)
        if "fm" in kinds:
            seams.extend(range(m, m + n, FM_TILE))
        if "sam" in kinds and n >= SAM_TILED_MIN:
            seams.extend(range(m, m + n, SAM_TILE))
        for kind in ("fm", "am", "sam"):
            cnt = kinds.count(kind) + (kinds.count("sam") if kind == "am" and n >= SAM_TILED_MIN else 0)
            if kinds.count(kind) and not (kind == "sam" and n < SAM_TILED_MIN):       # (short SAM calls take the sequential kernel)
                S, batches = 16 * seg_groups(cnt, n), (n + 63) // 64
                seams.extend(m + 64 * (w * batches // S) for w in range(S))
        m += n
    return np.unique(np.array(seams, dtype=np.int64)), np.array(calls, dtype=np.int64)


def margins(got, rec, seams, calls):
    w = worst_sample(got, rec["want"], rec["bound"], seams, calls)
    g = np.asarray(got).astype(np.complex128)
    err = np.maximum(np.abs(g.real - rec["want"].real), np.abs(g.imag - rec["want"].imag)).max(axis=1)
    w["err_over_E"] = float(max(float(e) / E for e, E in zip(err, rec["E"])))
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# running a case: on the engine, and on the oracle
# ---------------------------------------------------------------------------------------------------------------------------
MODE = {"usb": USB, "am": AM, "sam": SAM, "fm": FM}


def _setup(call, c, ch):
    call("SetRXAShiftRun", c, 1)
    call("SetRXAShiftFreq", c, SHIFTS[ch.idx % 3])
    call("RXANBPSetRun", c, 1)
    call("SetRXAMode", c, USB)                                  # from LSB, the mode a channel is made in: the change takes bp1 out (RXA.c:748-787)
    call("RXASetPassband", c, *BANDS[ch.kind])                  # the detector's own passband, ahead of the prime blocks
    call("SetRXAAGCMode", c, 0)
    call("SetRXAAGCFixed", c, AGC_DB)
    if ch.kind in ("am", "sam"):
        call("SetRXAAMDFadeLevel", c, ch.levelfade)
        call("SetRXAAMDSBMode", c, ch.sbmode)
    if ch.kind == "fm":
        call("SetRXAFMDeviation", c, ch.deviation)
        call("SetRXACTCSSFreq", c, ch.ctcss_freq)
        call("SetRXACTCSSRun", c, ch.ctcss_run)
        if ch.nc_de != NC:
            call("SetRXAFMNCde", c, ch.nc_de)
        if ch.nc_aud != NC:
            call("SetRXAFMNCaud", c, ch.nc_aud)


def run_engine(qh, chans, schedule, meters=False, info=None):
    """The case on a fresh RxaEngine: the prime blocks as one call in USB mode, SetRXAMode, then the schedule's calls.  Returns the
    outputs behind the switch [nch, m]; info takes the repair count."""
    rec = case_ref(tuple(chans), tuple(schedule))
    e = qh.RxaEngine(len(chans), dsp_size=DSP_SIZE, in_rate=IN_RATE, dsp_rate=DSP_RATE, out_rate=DSP_RATE)
    try:
        def call(name, c, *args):
            getattr(e, name)(c, *args)
        for c, ch in enumerate(chans):
            _setup(call, c, ch)
        if meters:
            e.enable_meters(True)
        x = rec["x"]
        e.process_host(np.ascontiguousarray(x[:, :PRIME * PER_IN]))
        for c, ch in enumerate(chans):
            e.SetRXAMode(c, MODE[ch.kind])
        out, pos = [], PRIME * PER_IN
        for nb in schedule:
            out.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * PER_IN])))
            pos += nb * PER_IN
        assert pos == x.shape[1]
        if info is not None:
            info.update(pll_repairs=e.pll_repairs())
        return np.concatenate(out, axis=1)
    finally:
        e.close()


def run_oracle(po, ch, schedule, turned=False):
    """The channel on oracle.WdspChannel with the same primed schedule: (the detector's own output at HOOK_FMSQ, xrxa's) behind the switch.
    turned: the oracle's oscillator (WDSP's recurrence in doubles, shift.c) is parked and the input is turned in long double ahead of it."""
    o = po.WdspChannel(PER_IN, DSP_SIZE, IN_RATE, DSP_RATE, DSP_RATE)

    def call(name, _c, *args):
        getattr(o, name)(*args)
    _setup(call, 0, ch)
    x = make_input(ch.kind, ch.idx)
    if turned:
        o.SetRXAShiftRun(0)
        x = (x.astype(CLD) * R.rotation(_phase(ch.idx, x.size))).astype(np.complex128)
    o.xrxa(x[:PRIME * PER_IN])
    o.SetRXAMode(MODE[ch.kind])
    taps = []
    o.set_stage_hook(lambda where, z, aux: taps.append(z.copy()), sites=(po.WdspChannel.HOOK_FMSQ,))
    out, pos = [], PRIME * PER_IN
    for nb in schedule:
        out.append(o.xrxa(x[pos:pos + nb * PER_IN]))
        pos += nb * PER_IN
    o.set_stage_hook(None)
    o.close()
    return np.concatenate(taps), np.concatenate(out)


# the channels of the GPU runs (tests/test_gpu_rxa_detector_forms.py) and of the CPU checks
FM3 = tuple(chan("fm", i) for i in range(3))
AM3 = (chan("am", 0), chan("am", 1, levelfade=0), chan("am", 2))
SAM3 = tuple(chan("sam", i, sbmode=i) for i in range(3))
SAM3_PLAIN = tuple(chan("sam", i, sbmode=i, levelfade=0) for i in range(3))
SAM3_COLD = tuple(chan("sam", 3 + i, sbmode=i) for i in range(3))
MIXED9 = tuple(chan(("usb", "am", "fm")[c % 3], c // 3) for c in range(9))
