"""What the GPU tests of the RXA engine's sender and siphon taps share: the five-mode engine of tests/test_gpu_rxa_ssql.py, an input with
tones and a noise floor inside every channel's passband, the oracle channel of a mode with a capture at one of its hook sites, and the
issue's ragged calls (17 blocks of 256 overrun the siphon's 4096-sample ring in one call; the others wrap it)."""
import numpy as np

from quisk_amd import synth

FS = 192000
DSP_RATE = 48000
MODES = [1, 0, 4, 6, 5]                                     # USB, LSB, CWU, AM, FM
CALLS = (3, 1, 17, 7, 7, 2)                                 # DSP blocks per call


def passband(mode):
    return (-8000.0, 8000.0) if mode == 5 else (-4000.0, 4000.0) if mode in (6, 10) else (-3000.0, -300.0) if mode in (0, 3, 9) else (300.0, 3000.0)


def engine(qh, modes, dsp_size=256):
    e = qh.RxaEngine(len(modes), dsp_size=dsp_size, in_rate=FS, dsp_rate=DSP_RATE, out_rate=DSP_RATE)
    for c, m in enumerate(modes):
        e.SetRXAShiftRun(c, 1); e.SetRXAShiftFreq(c, synth.shift_freq(c)); e.RXANBPSetRun(c, 1)
        e.SetRXAMode(c, m)
        e.RXASetPassband(c, *passband(m))
    if dsp_size > 2048:
        e.RXASetNC(-1, dsp_size)                            # create_rxa's nc is max(2048, dsp_size) (RXA.c:96), the engine's 2048
    return e


def signal(modes, n, seed=0):
    """[nch, n] complex128 at FS: per channel two tones and a noise floor that land inside its passband behind the shift (SSB / CW), on a
    carrier with 40 % AM, or as +-3 kHz FM"""
    t = np.arange(n) / FS
    x = np.empty((len(modes), n), dtype=np.complex128)
    for c, m in enumerate(modes):
        rng = np.random.default_rng(seed + 17 * c)
        f1, f2 = 700.0 + 31.0 * c, 1900.0 - 53.0 * c
        z = 0.2 * np.exp(2j * np.pi * ((f1 * t) % 1.0)) + 0.05 * np.exp(2j * np.pi * ((f2 * t) % 1.0))
        car = np.exp(-2j * np.pi * ((synth.shift_freq(c) * t) % 1.0))
        floor = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.003
        if m == 6:
            x[c] = (0.1 + 0.16 * z.real) * car + floor
        elif m == 5:
            x[c] = 0.1 * np.exp(2j * np.pi * np.cumsum(3000.0 * z.real / 0.25) / FS) * car + floor
        else:
            x[c] = (z if m in (0, 3, 9) else np.conj(z)) * car + floor         # WDSP's +f is exp(-j 2 pi f t) of I + jQ (fir.c's impulses)
    return x


def oracle_channel(oracle, c, mode, dsp_size=256, nbp_only=False):
    """the oracle's channel c in `mode`; nbp_only: in USB mode with channel c's shift and `mode`'s passband on nbp0 alone -- nothing ahead of
    xamd depends on the mode, so midbuff at HOOK_FMSQ is then nbp0's output (oracle/wdsp_oracle.c:1126-1132)"""
    o = oracle.WdspChannel(4 * dsp_size, dsp_size, FS, DSP_RATE, DSP_RATE)
    o.SetRXAShiftRun(1); o.SetRXAShiftFreq(synth.shift_freq(c)); o.RXANBPSetRun(1)
    if nbp_only:
        o.SetRXAMode(1)
        o.RXANBPSetFreqs(*passband(mode))
    else:
        o.SetRXAMode(mode)
        o.RXASetPassband(*passband(mode))
    return o


def capture(o, site, x):
    """(midbuff at the hook site over the blocks of x, the channel's output)"""
    got = []
    o.set_stage_hook(lambda where, z, aux: got.append(z.copy()), sites=(site,))
    y = o.xrxa(x)
    o.set_stage_hook(None)
    return np.concatenate(got), y


# ---- the display of the attach tests: size 1024, buffers of 256 (= dsp_size), overlap 512, 400 pixels, peak detector, no averaging.
# The window is the rectangular one (type 0).  The signal behind nbp0 has a stop band 150 dB down, and the display keeps floats: with a
# Hann window the stop band's pixels (-172 dB) are the window's far skirt, 40 dB above what ONE float ulp of ONE sample spreads over the
# bins (-211 dB), so two inputs that agree to 1e-11 as doubles and differ in two of 9472 floats by an ulp move those pixels by a tenth of
# a dB.  Measured with Hann: the attached bank 0.246 dB and 17.8 % of the pixels off the oracle's on the CWU channel (0 on the two
# channels whose floats all agree), GetPixels through the WDSP names 0.389 dB and 3.8 %; the same bank fed from the host with np.float32 of
# the oracle's own signal: 0.0 on every channel -- the input's last bits, not the plumbing.  Under the rectangular window every pixel is
# leakage of the tones, 100 dB and more above an ulp: the gates measure the display path.
STEP = 0.0022
SIZE, BF, OVERLAP, NPIX = 1024, 256, 512, 400
WINDOW = 0
ARGS = (1, 1, 1, [0], SIZE, BF, WINDOW, 0.0, OVERLAP, 0, 0.0, 0.0, NPIX, 1, 0, 0.0, 0.0, 2 * SIZE)


def compare_rows(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got - want)
    print(what, "max", d.max(), "share above 1e-4 dB", np.mean(d > 1e-4))
    assert d.max() < STEP, (what, d.max(), int(d.argmax()))
    assert np.mean(d > 1e-4) < 0.02, (what, np.mean(d > 1e-4))


def oracle_rows(oracle, z):
    """every row GetPixels hands out while z (the chain's I + jQ) goes in block by block as xsender hands it over: (I, Q) pairs"""
    a = oracle.OracleAnalyzer(SIZE, 1)
    a.SetDisplaySampleRate(DSP_RATE)
    a.SetAnalyzer(*ARGS)
    rows = []
    for b in range(z.size // BF):
        blk = z[b * BF:(b + 1) * BF]
        buf = np.empty(2 * BF); buf[0::2] = blk.real; buf[1::2] = blk.imag
        a.Spectrum0(1, 0, 0, buf)
        pix, flag = a.GetPixels(0)
        if flag:
            rows.append(pix)
    return np.array(rows)
