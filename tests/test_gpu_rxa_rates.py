"""channel.c's run-time rate and buffer-size setters on a live engine (qh_rxa_set_in_rate / _out_rate / _dsp_rate / _dsp_size / _rates,
wdsp/channel.c:169-258 with RXA.c:600-740): which state runs on and which starts from zero, against references composed from oracle
pieces only.  dsp_size 64, default nc 2048, three channels, calls of 2 to 5 DSP blocks; the gate is relative RMS <= 1e-6 (fp64) over the
output behind the change.  -m gpu.

  input rate   the oracle channel is opened at in = dsp rate and runs on; wo_resample objects with create_rxa's rsmpin arguments (RXA.c:48-57)
               stand in front of it, the old one up to the change and a fresh one behind it.  A reference that starts the channel afresh
               at the change is shown to miss the engine at the AGC, so the gate pins "the DSP-rate state runs on".
  output rate  the same with rsmpout: the oracle channel is opened with out = dsp, a fresh wo_resample follows it behind the change.
  dsp rate /   a signal, then silence until every kept delay line rests, then the change, then a signal: a fresh reference channel
  dsp size     (rxa_chain_ref.RxaChainRef: the oracle with the restated xfmsq, xeqp, xspeak and xssql hooked in) at the new values with the
               same setter list.  The FM detector's audio dies away as exp(-t / 0.02 s) in silence (fmdc, fmd.c:154-157), so the de-emphasis
               filter's kept line only rests near zero: the silence before a new dsp_rate is 0.6 s (e^-30).  The AM detector's fade leveller
               puts dc_insert - dc out in silence, and dc_insert has tau 1.4 s (amd.c:86-89,152-157): it rests in no silence a test can
               afford.  A new dsp_rate keeps bp1's delay line, which holds that output (measured with the leveller on: 0.03 and 0.06 rel RMS
               against the fresh channel, the tail of the kept line), and setSize_amd keeps the averages themselves (amd.c:253-256).  So the
               AM channel of these two cases runs with the fade leveller off: the detector then puts out exact zeros in silence and nothing
               reads the averages.
  FM           a loop that starts on the rounding-sized samples of filters still filling is no continuous function of its input and no one's
               to compare: the FM channel runs its first LEAD blocks in USB and enters FM with its filters primed, at
               the start and again behind a change that starts the filters from zero.
  kept lines   USB, fixed AGC, nbp0 alone, dsp_rate 48 k -> 96 k in mid-signal: the fresh channel's output plus what nbp0's new impulse
               response makes of the old delay line, through the panel's gain and a fresh rsmpout.  And AM with the leveller off: nbp0's
               and bp1's kept lines with the detector between them, the chain composed from wo_fircore pieces.
  gen0         the tone's phase runs on across a new dsp_size (setSize_gen), against the restated generator in front of a fresh channel.
"""
import numpy as np
import pytest
import torch

from conftest import rel_rms
from rxa_chain_ref import RxaChainRef

pytestmark = pytest.mark.gpu

SIZE, GATE = 64, 1e-6
USB, FM, AM = 1, 5, 6
KINDS = ("usb", "am", "fm")
MODES = {"usb": USB, "am": AM, "fm": FM}
BANDS = {"usb": (300.0, 3000.0), "am": (-4000.0, 4000.0), "fm": (-4000.0, 4000.0)}
CALLS = (2, 5, 3, 4)


def signal(kind, n, fs, seed, fo=0.0):
    """n samples at fs of a carrier at fo: USB tones 1 kHz below it and 7 kHz above, AM with m = 0.5 at 1 kHz, FM with 3 kHz deviation at 1 kHz"""
    t = np.arange(n, dtype=np.float64) / fs
    g = np.random.default_rng(seed).standard_normal((n, 2))
    noise = 0.01 * (g[:, 0] + 1j * g[:, 1])
    car = np.exp(2j * np.pi * fo * t)
    if kind == "usb":
        return 0.1 * np.exp(2j * np.pi * (fo - 1000.0) * t) + 0.05 * np.exp(2j * np.pi * (fo + 7000.0) * t) + noise
    if kind == "am":
        return 0.1 * (1.0 + 0.5 * np.cos(2 * np.pi * 1000.0 * t)) * car + noise
    return 0.1 * car * np.exp(3j * np.sin(2 * np.pi * 1000.0 * t)) + noise


def signals(nblk, fs, dsp_rate, seed, fo=0.0):
    return np.stack([signal(k, nblk * SIZE * fs // dsp_rate, fs, seed + i, fo) for i, k in enumerate(KINDS)])


LEAD = 40       # blocks an FM channel spends in USB while its filters fill (nc = 2048 is 32 blocks)


def base_setters(kind, shift=0.0, primed=True):
    """primed False: the FM channel's settings with USB for its mode, until enter_fm"""
    mode = USB if kind == "fm" and not primed else MODES[kind]
    return [("SetRXAMode", mode), ("RXASetPassband",) + BANDS[kind], ("SetRXAShiftRun", 1), ("SetRXAShiftFreq", shift), ("RXANBPSetRun", 1)]


def enter_fm(target, ch, kind):
    if kind == "fm":
        apply(target, ch, [("SetRXAMode", FM)])


def apply(target, ch, setters):
    for name, *args in setters:
        getattr(target, name)(*(([ch] if ch is not None else []) + args))


def run(e, x):
    """x through the engine in calls of 2 to 5 DSP blocks"""
    per, out, pos, i = e.dsp_insize, [], 0, 0
    assert x.shape[1] % per == 0
    nblk = x.shape[1] // per
    while pos < nblk:
        k = min(CALLS[i % len(CALLS)], nblk - pos)
        out.append(e.process_host(x[:, pos * per:(pos + k) * per]))
        pos, i = pos + k, i + 1
    return np.concatenate(out, axis=1)


def front(po, x, rate, dsp_rate=48000):
    return x if rate == dsp_rate else po.Resample(rate, dsp_rate)(x)


def report(name, errs):
    print("%s: worst rel RMS %.3e (%s)" % (name, max(errs), ", ".join("%.2e" % v for v in errs)))


NB1, NB2 = 47, 61


def primed_engine(qh, x0, **kw):
    e = qh.RxaEngine(3, dsp_size=SIZE, **kw)
    for c, k in enumerate(KINDS):
        apply(e, c, base_setters(k, primed=False))
    run(e, x0)
    for c, k in enumerate(KINDS):
        enter_fm(e, c, k)
    return e


def primed_oracle(oracle, k, m0):
    o = oracle.WdspChannel(SIZE, SIZE, 48000, 48000, 48000)
    apply(o, None, base_setters(k, primed=False))
    o.xrxa(m0)
    enter_fm(o, None, k)
    return o


@pytest.mark.parametrize("r1,r2", [(192000, 96000), (48000, 192000)])
def test_a_new_input_rate_leaves_the_dsp_rate_state_running(qh, oracle, r1, r2):
    x0, x1, x2 = signals(LEAD, r1, 48000, 50), signals(NB1, r1, 48000, 100), signals(NB2, r2, 48000, 200)
    e = primed_engine(qh, x0, in_rate=r1, dsp_rate=48000, out_rate=48000)
    y1 = run(e, x1)
    e.set_in_rate(r2)
    assert (e.in_rate, e.dsp_rate, e.out_rate, e.dsp_size) == (r2, 48000, 48000, SIZE)
    assert e.dsp_insize == SIZE * r2 // 48000 and e.dsp_outsize == SIZE
    y2 = run(e, x2)
    e.close()
    errs, fresh = [], []
    for c, k in enumerate(KINDS):
        old = oracle.Resample(r1, 48000) if r1 != 48000 else (lambda v: v)
        o = primed_oracle(oracle, k, old(x0[c]))
        m1, m2 = old(x1[c]), front(oracle, x2[c], r2)
        assert m1.size == NB1 * SIZE and m2.size == NB2 * SIZE
        ref = o.xrxa(np.concatenate([m1, m2]))
        assert rel_rms(y1[c], ref[:NB1 * SIZE]) <= GATE
        errs.append(rel_rms(y2[c], ref[NB1 * SIZE:]))
        o2 = oracle.WdspChannel(SIZE, SIZE, 48000, 48000, 48000)
        apply(o2, None, base_setters(k))
        fresh.append(rel_rms(y2[c], o2.xrxa(m2)))
    report("in_rate %d -> %d" % (r1, r2), errs)
    assert max(errs) <= GATE
    assert fresh[0] > 1e-3, "a channel made afresh at the change should miss the engine at the AGC: %r" % (fresh,)


def test_a_new_input_rate_restarts_the_shift_at_phase_zero(qh, oracle):
    r1, r2, f = 192000, 96000, 10000.0
    kinds = ("usb", "am")
    x1 = np.stack([signal(k, NB1 * SIZE * 4, r1, 300 + i, -f) for i, k in enumerate(kinds)])
    x2 = np.stack([signal(k, NB2 * SIZE * 2, r2, 400 + i, -f) for i, k in enumerate(kinds)])
    e = qh.RxaEngine(2, dsp_size=SIZE, in_rate=r1, dsp_rate=48000, out_rate=48000)
    for c, k in enumerate(kinds):
        apply(e, c, base_setters(k, f))
    y1 = run(e, x1)
    e.set_in_rate(r2)
    y2 = run(e, x2)
    e.close()

    def xshift(x, rate):        # shift.c:60-85 from phase 0 (setSamplerate_shift, shift.c:93-98)
        return x * np.exp(1j * (2.0 * np.pi * f / rate) * np.arange(x.size))
    errs = []
    for c, k in enumerate(kinds):
        o = oracle.WdspChannel(SIZE, SIZE, 48000, 48000, 48000)
        apply(o, None, base_setters(k))
        o.SetRXAShiftRun(0)
        ref = o.xrxa(np.concatenate([front(oracle, xshift(x1[c], r1), r1), front(oracle, xshift(x2[c], r2), r2)]))
        assert rel_rms(y1[c], ref[:NB1 * SIZE]) <= GATE
        errs.append(rel_rms(y2[c], ref[NB1 * SIZE:]))
    report("in_rate 192000 -> 96000, shift 10 kHz", errs)
    assert max(errs) <= GATE


@pytest.mark.parametrize("r2", [96000, 24000])
def test_a_new_output_rate_touches_rsmpout_alone(qh, oracle, r2):
    x0, x = signals(LEAD, 48000, 48000, 450), signals(NB1 + NB2, 48000, 48000, 500)
    e = primed_engine(qh, x0, in_rate=48000, dsp_rate=48000, out_rate=48000)
    y1 = run(e, x[:, :NB1 * SIZE])
    e.set_out_rate(r2)
    assert (e.in_rate, e.dsp_rate, e.out_rate) == (48000, 48000, r2) and e.dsp_outsize == SIZE * r2 // 48000 and e.dsp_insize == SIZE
    y2 = run(e, x[:, NB1 * SIZE:])
    e.close()
    errs = []
    for c, k in enumerate(KINDS):
        mid = primed_oracle(oracle, k, x0[c]).xrxa(x[c])
        assert rel_rms(y1[c], mid[:NB1 * SIZE]) <= GATE
        ref = oracle.Resample(48000, r2)(mid[NB1 * SIZE:])
        assert ref.size == y2[c].size
        errs.append(rel_rms(y2[c], ref))
    report("out_rate 48000 -> %d" % r2, errs)
    assert max(errs) <= GATE


# a setter list that touches every stage family: notches, bp1 forced on by AM, AGC times, AMSQ, FMSQ, EQ, a peak filter, SSQL, ANF
WALK = {
    "usb": [("RXANBPAddNotch", 0, 1500.0, 200.0, 1), ("RXANBPSetNotchesRun", 1), ("SetRXAEQRun", 1),
            ("SetRXAGrphEQ10", [3, -6, -3, 0, 2, 4, 6, 3, 0, -3, -6]), ("SetRXASPCWRun", 1), ("SetRXASPCWFreq", 1000.0), ("SetRXASSQLRun", 1),
            ("SetRXAANFRun", 1)],
    "am": [("SetRXAAGCAttack", 2), ("SetRXAAGCDecay", 300), ("SetRXAAGCHang", 100), ("SetRXAAMSQRun", 1), ("SetRXAAMSQThreshold", -60.0)],
    "fm": [("SetRXAFMSQThreshold", 0.5)],       # and SetRXAFMSQRun with the mode: the engine refuses an FM squelch without its detector
}
LEVEL_OFF = {"am": [("SetRXAAMDFadeLevel", 0)]}
FM_ON, FM_OFF = [("SetRXAMode", FM), ("SetRXAFMSQRun", 1)], [("SetRXAFMSQRun", 0), ("SetRXAMode", USB)]


def walked_engine(qh, in_rate, dsp_rate, out_rate, size, extra):
    e = qh.RxaEngine(3, dsp_size=size, in_rate=in_rate, dsp_rate=dsp_rate, out_rate=out_rate)
    for c, k in enumerate(KINDS):
        apply(e, c, base_setters(k) + WALK[k] + extra.get(k, []) + (FM_ON if k == "fm" else []))
        e.SetRXAPreGenRun(c, 0)
    return e


def walked_reference(k, in_rate, dsp_rate, out_rate, size, extra):
    r = RxaChainRef(size * in_rate // dsp_rate, size, in_rate, dsp_rate, out_rate)
    apply(r, None, base_setters(k, primed=False) + WALK[k] + extra.get(k, []))
    return r


def after_silence(qh, before, after, change, nsilent, extra):
    """signal, silence, change(engine), signal: the worst rel RMS behind the change against fresh references at `after`, per channel"""
    (in1, dsp1, out1, size1), (in2, dsp2, out2, size2) = before, after
    e = walked_engine(qh, in1, dsp1, out1, size1, extra)
    nb1, nb2 = 40 * SIZE // size1, 80 * SIZE // size2
    x1 = np.stack([signal(k, nb1 * size1 * in1 // dsp1, in1, 600 + i) for i, k in enumerate(KINDS)])
    run(e, x1)
    run(e, np.zeros((3, nsilent * size1 * in1 // dsp1), dtype=np.complex128))
    apply(e, KINDS.index("fm"), FM_OFF)         # the FM channel comes back to FM once the filters the change empties have filled
    change(e)
    assert (e.in_rate, e.dsp_rate, e.out_rate, e.dsp_size) == after
    assert e.dsp_insize == size2 * in2 // dsp2 and e.dsp_outsize == size2 * out2 // dsp2
    lead = LEAD * SIZE // size2 * dsp2 // 48000
    x0 = np.stack([signal(k, lead * size2 * in2 // dsp2, in2, 650 + i) for i, k in enumerate(KINDS)])
    x2 = np.stack([signal(k, nb2 * size2 * in2 // dsp2, in2, 700 + i) for i, k in enumerate(KINDS)])
    y0 = run(e, x0)
    apply(e, KINDS.index("fm"), FM_ON)
    y2 = run(e, x2)
    e.close()
    errs = []
    for c, k in enumerate(KINDS):
        r = walked_reference(k, in2, dsp2, out2, size2, extra)
        r0 = r.xrxa(x0[c])
        apply(r, None, FM_ON if k == "fm" else [])
        errs.append(max(rel_rms(y0[c], r0), rel_rms(y2[c], r.xrxa(x2[c]))))
        assert r.margins_ok(), (k, r.margins())
        r.close()
    return errs


@pytest.mark.parametrize("dsp1,dsp2", [(48000, 96000), (96000, 48000)])
def test_a_new_dsp_rate_after_silence_equals_a_fresh_channel(qh, oracle, dsp1, dsp2):
    errs = after_silence(qh, (96000, dsp1, 48000, SIZE), (96000, dsp2, 48000, SIZE), lambda e: e.set_dsp_rate(dsp2), int(0.6 * dsp1) // SIZE, LEVEL_OFF)
    report("dsp_rate %d -> %d after silence" % (dsp1, dsp2), errs)
    assert max(errs) <= GATE


def test_a_new_dsp_size_after_silence_equals_a_fresh_channel(qh, oracle):
    errs = after_silence(qh, (96000, 48000, 48000, SIZE), (96000, 48000, 48000, 128), lambda e: e.set_dsp_size(128), 48, LEVEL_OFF)
    report("dsp_size 64 -> 128 after silence", errs)
    assert max(errs) <= GATE


def test_set_rates_with_the_dsp_rate_unchanged_is_an_input_and_an_output_rate_change(qh, oracle):
    r1, r2, o2 = 192000, 96000, 96000
    x0, x1, x2 = signals(LEAD, r1, 48000, 750), signals(NB1, r1, 48000, 800), signals(NB2, r2, 48000, 900)
    e = primed_engine(qh, x0, in_rate=r1, dsp_rate=48000, out_rate=48000)
    run(e, x1)
    e.set_rates(r2, 48000, o2)
    y2 = run(e, x2)
    e.close()
    errs = []
    for c, k in enumerate(KINDS):
        old = oracle.Resample(r1, 48000)
        o = primed_oracle(oracle, k, old(x0[c]))
        mid = o.xrxa(np.concatenate([old(x1[c]), front(oracle, x2[c], r2)]))
        errs.append(rel_rms(y2[c], oracle.Resample(48000, o2)(mid[NB1 * SIZE:])))
    report("set_rates 192000/48000/48000 -> 96000/48000/96000", errs)
    assert max(errs) <= GATE


def test_a_new_dsp_rate_keeps_nbp0s_delay_line(qh, oracle):
    nc, gain1 = 2048, 4.0
    sets = [("SetRXAMode", USB), ("RXASetPassband", 300.0, 3000.0), ("SetRXAShiftRun", 0), ("RXANBPSetRun", 1), ("SetRXAAGCMode", 0), ("SetRXAAGCFixed", 0.0)]
    x1, x2 = signal("usb", NB1 * SIZE * 2, 96000, 1000), signal("usb", NB2 * SIZE, 96000, 1001)
    e = qh.RxaEngine(1, dsp_size=SIZE, in_rate=96000, dsp_rate=48000, out_rate=48000)
    apply(e, 0, sets)
    run(e, x1[None, :])
    e.set_dsp_rate(96000)
    assert e.dsp_insize == SIZE and e.dsp_outsize == SIZE // 2
    y2 = run(e, x2[None, :])[0]
    e.close()
    o = oracle.WdspChannel(SIZE, SIZE, 96000, 96000, 48000)
    apply(o, None, sets)
    fresh = o.xrxa(x2)
    # nbp0's line: the front's output before the change; its new impulse response (calc_nbp_impulse at 96 kHz, nbp.c:221-238) runs over it
    line = oracle.Resample(96000, 48000)(x1)[-nc:]
    h = oracle.fir_bandpass(nc, 300.0, 3000.0, 96000.0, 0, 1, 1.0 / (2.0 * SIZE))
    tail = oracle.Fircore(SIZE, nc, h)(np.concatenate([line, np.zeros(NB2 * SIZE, dtype=np.complex128)]))[nc:]
    ref = fresh + oracle.Resample(96000, 48000)(gain1 * tail)
    err, without = rel_rms(y2, ref), rel_rms(y2, fresh)
    print("kept nbp0 line, dsp_rate 48000 -> 96000: rel RMS %.3e (against the fresh channel alone %.3e)" % (err, without))
    assert err <= GATE
    assert without > 1e-3, "the old line's tail should be audible"


def test_a_new_dsp_rate_keeps_bp1s_delay_line_behind_the_am_detector(qh, oracle):
    """AM with the fade leveller off and a fixed AGC, dsp_rate 48 k -> 96 k in mid-signal: nbp0 and bp1 both run their new impulse responses
    over the lines they held (nbp.c:298-304, bandpass.c:334-341), the detector between them has no state in this form (amd.c:139-165).  The
    chain is composed from its pieces -- wo_fircore with wo_fir_bandpass designs, |z| on both rails, the panel's gain, a fresh rsmpout --,
    which equals the oracle's AM channel to 1.5e-16 where nothing changes.  A reference with bp1's line zeroed is shown to miss."""
    nc = 2048
    sets = [("SetRXAMode", AM), ("RXASetPassband", -4000.0, 4000.0), ("SetRXAShiftRun", 0), ("RXANBPSetRun", 1), ("SetRXAAGCMode", 0),
            ("SetRXAAGCFixed", 0.0), ("SetRXAAMDFadeLevel", 0)]
    x1, x2 = signal("am", NB1 * SIZE * 2, 96000, 1500), signal("am", NB2 * SIZE, 96000, 1501)
    e = qh.RxaEngine(1, dsp_size=SIZE, in_rate=96000, dsp_rate=48000, out_rate=48000)
    apply(e, 0, sets)
    y1 = run(e, x1[None, :])[0]
    e.set_dsp_rate(96000)
    y2 = run(e, x2[None, :])[0]
    e.close()

    def design(rate, wintype, gain):
        return oracle.fir_bandpass(nc, -4000.0, 4000.0, float(rate), wintype, 1, gain / (2.0 * SIZE))

    def detect(z):
        return np.abs(z) * (1.0 + 1.0j)
    m1 = oracle.Resample(96000, 48000)(x1)
    a1 = detect(oracle.Fircore(SIZE, nc, design(48000, 0, 1.0))(m1))
    assert rel_rms(y1, 4.0 * oracle.Fircore(SIZE, nc, design(48000, 1, 2.0))(a1)) <= GATE
    a2 = detect(oracle.Fircore(SIZE, nc, design(96000, 0, 1.0))(np.concatenate([m1[-nc:], x2]))[nc:])
    bp1 = design(96000, 1, 2.0)             # RXAbp1Check: gain 2 behind the AM detector (RXA.c:800-812)
    kept = oracle.Fircore(SIZE, nc, bp1)(np.concatenate([a1[-nc:], a2]))[nc:]
    err = rel_rms(y2, oracle.Resample(96000, 48000)(4.0 * kept))
    zeroed = rel_rms(y2, oracle.Resample(96000, 48000)(4.0 * oracle.Fircore(SIZE, nc, bp1)(a2)))
    print("kept nbp0 and bp1 lines in AM, dsp_rate 48000 -> 96000: rel RMS %.3e (with bp1's line zeroed %.3e)" % (err, zeroed))
    assert err <= GATE
    assert zeroed > 1e-3


def test_a_new_dsp_size_leaves_gen0_s_phase_running(qh, oracle):
    """setSize_gen writes the size and flushes the pulse's state alone (gen.c:160-163,369-373): the tone goes on from the phase it has
    reached, while everything behind it starts from zero.  Reference: the restated gen0 (wdsp_gen_ref.Gen), its size changed and flushed
    in mid-stream, in front of a fresh oracle channel at the new size.  103 blocks of 1234.5 Hz end 0.54 of a turn into the tone: a
    generator that started again is shown to miss the engine."""
    from wdsp_gen_ref import Gen
    nb1, nb2, f = 103, 40, 1234.5
    sets = [("SetRXAMode", USB), ("RXASetPassband", 300.0, 3000.0), ("SetRXAShiftRun", 0), ("RXANBPSetRun", 1), ("SetRXAAGCMode", 0), ("SetRXAAGCFixed", 0.0)]
    e = qh.RxaEngine(1, dsp_size=SIZE, in_rate=48000, dsp_rate=48000, out_rate=48000)
    apply(e, 0, sets + [("SetRXAPreGenMode", 0), ("SetRXAPreGenToneFreq", f), ("SetRXAPreGenToneMag", 0.1), ("SetRXAPreGenRun", 1)])
    run(e, np.zeros((1, nb1 * SIZE), dtype=np.complex128))
    e.set_dsp_size(128)
    y2 = run(e, np.zeros((1, nb2 * 128), dtype=np.complex128))[0]
    e.close()
    g = Gen(48000, SIZE, run=1, mode=0)
    g.SetToneFreq(f); g.SetToneMag(0.1)
    for _ in range(nb1):
        g.block()
    g.size = 128
    g.flush()
    x2 = np.concatenate([g.block() for _ in range(nb2)])
    o = oracle.WdspChannel(128, 128, 48000, 48000, 48000)
    apply(o, None, sets)
    err = rel_rms(y2, o.xrxa(x2))
    g0 = Gen(48000, 128, run=1, mode=0)
    g0.SetToneFreq(f); g0.SetToneMag(0.1)
    o0 = oracle.WdspChannel(128, 128, 48000, 48000, 48000)
    apply(o0, None, sets)
    restarted = rel_rms(y2, o0.xrxa(np.concatenate([g0.block() for _ in range(nb2)])))
    print("gen0 across dsp_size 64 -> 128: rel RMS %.3e (against a generator started again %.3e)" % (err, restarted))
    assert err <= GATE
    assert restarted > 1e-2


def ptr_run(e, x, d_in, d_out, nblk):
    """x through the engine nblk blocks at a time, from and to the same two device buffers (what the launch-sequence replay needs)"""
    per, out = e.dsp_insize * nblk, []
    for b in range(x.shape[1] // per):
        d_in[:, :per].copy_(torch.from_numpy(x[:, b * per:(b + 1) * per]))
        torch.cuda.synchronize()
        e.process_ptr(d_in.data_ptr(), d_in.shape[1], d_out.data_ptr(), d_out.shape[1], nblk)
        e.synchronize()
        out.append(d_out[:, :nblk * e.dsp_outsize].cpu().numpy().copy())
    return np.concatenate(out, axis=1)


def pair(qh, replay, **kw):
    dev = torch.device("cuda:0")
    es = []
    for r in replay:
        e = qh.RxaEngine(3, dsp_size=SIZE, **kw)
        for c, k in enumerate(KINDS):
            apply(e, c, base_setters(k))
        e.set_graph_replay(r)
        es.append((e, torch.zeros((3, 2 * SIZE * 4), dtype=torch.complex128, device=dev), torch.zeros((3, 2 * SIZE * 2), dtype=torch.complex128, device=dev)))
    return es


def test_a_call_that_changes_nothing_does_nothing(qh):
    x = signals(24, 192000, 48000, 1100)
    (a, a_in, a_out), (b, b_in, b_out) = pair(qh, (True, True), in_rate=192000, dsp_rate=48000, out_rate=48000)
    half = 12 * SIZE * 4
    ya = [ptr_run(a, x[:, :half], a_in, a_out, 2)]
    yb = [ptr_run(b, x[:, :half], b_in, b_out, 2)]
    before = a.graph_launches()
    assert before > 0
    a.set_rates(192000, 48000, 48000); a.set_in_rate(192000); a.set_dsp_rate(48000); a.set_out_rate(48000); a.set_dsp_size(SIZE)
    ya.append(ptr_run(a, x[:, half:], a_in, a_out, 2))
    yb.append(ptr_run(b, x[:, half:], b_in, b_out, 2))
    assert np.array_equal(np.concatenate(ya, axis=1), np.concatenate(yb, axis=1))
    assert a.graph_launches() == b.graph_launches() == before + 6      # every later call is replayed: nothing was dropped
    a.close(); b.close()


def test_a_refused_change_changes_nothing(qh):
    x = signals(24, 96000, 48000, 1200)
    (a, a_in, a_out), (b, b_in, b_out) = pair(qh, (False, False), in_rate=96000, dsp_rate=48000, out_rate=48000)
    half = 12 * SIZE * 2
    ya = [ptr_run(a, x[:, :half], a_in, a_out, 2)]
    yb = [ptr_run(b, x[:, :half], b_in, b_out, 2)]
    state, nbytes = (a.in_rate, a.dsp_rate, a.out_rate, a.dsp_size, a.dsp_insize, a.dsp_outsize), a.device_bytes()
    with pytest.raises(qh.QuiskHipError):
        a.set_dsp_rate(64000)               # 96 k / 64 k is whole in neither direction (channel.c:39-42)
    with pytest.raises(qh.QuiskHipError):
        a.set_dsp_size(4096)                # above nc = 2048 (nbp.c:308)
    with pytest.raises(qh.QuiskHipError):
        a.set_rates(96000, 48000, 36000)
    with pytest.raises(qh.QuiskHipError):
        a.set_dsp_size(96)
    assert (a.in_rate, a.dsp_rate, a.out_rate, a.dsp_size, a.dsp_insize, a.dsp_outsize) == state and a.device_bytes() == nbytes
    ya.append(ptr_run(a, x[:, half:], a_in, a_out, 2))
    yb.append(ptr_run(b, x[:, half:], b_in, b_out, 2))
    assert np.array_equal(np.concatenate(ya, axis=1), np.concatenate(yb, axis=1))
    a.close(); b.close()


@pytest.mark.parametrize("what", ["in_rate", "dsp_rate"])
def test_replayed_calls_behind_a_change_equal_plain_launches(qh, what):
    x1 = signals(12, 192000, 48000, 1300)
    x2 = signals(24, 96000, 48000 if what == "in_rate" else 96000, 1400)
    ys, launches = [], []
    for e, d_in, d_out in pair(qh, (False, True), in_rate=192000, dsp_rate=48000, out_rate=48000):
        ptr_run(e, x1, d_in, d_out, 2)
        if what == "in_rate":
            e.set_in_rate(96000)
        else:
            e.set_rates(96000, 96000, 96000)
        ys.append(ptr_run(e, x2, d_in, d_out, 2))
        launches.append(e.graph_launches())
        e.close()
    assert np.all(np.isfinite(ys[0])) and np.abs(ys[0]).max() > 1e-3
    assert np.array_equal(ys[0], ys[1])
    assert launches[0] == 0 and launches[1] >= 5 + 9        # 6 replayed calls ahead of the change, 12 calls behind it of which 3 set up


def test_the_sizes_and_the_memory_follow_the_rates(qh):
    e = qh.RxaEngine(2, dsp_size=SIZE, in_rate=192000, dsp_rate=48000, out_rate=48000)
    x = np.zeros((2, 2 * SIZE * 4), dtype=np.complex128)
    e.process_host(x)
    full = e.device_bytes()
    e.set_in_rate(48000)                    # the overlap-save front stage's tables and delay lines are given back
    assert e.dsp_insize == SIZE and e.device_bytes() < full - 2 * 2 * 2240 * 16
    e.set_in_rate(192000)
    assert e.dsp_insize == 4 * SIZE and e.device_bytes() == full
    e.set_out_rate(24000)
    assert e.dsp_outsize == SIZE // 2
    e.set_dsp_size(128)
    assert (e.dsp_insize, e.dsp_outsize, e.dsp_size) == (512, 64, 128)
    assert e.process_host(np.zeros((2, 512), dtype=np.complex128)).shape == (2, 64)
    e.close()
