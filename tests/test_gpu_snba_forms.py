"""The two forms of xsnba against each other, bit for bit (qh_rxa_set_snba_form): the single kernel with both of the blanker's resamplers
inside its block loop, and the three passes -- decimation to 12 kHz for the whole call, the frames on 12 kHz rows, interpolation back --
that run the blanker at 96 to 384 kHz.  Where both can run (dsp_rate up to 48 kHz, dsp_size up to 1024) every sum has the same terms in
the same order without contraction in both, so every output sample and every meter agree in every bit: this pins the passes (windows,
histories across ragged calls, phases, per-channel taps) without going through the detector's thresholds.  -m gpu."""
import numpy as np
import pytest
import torch

from snba_rate_cases import AM, LSB, USB, Case

pytestmark = pytest.mark.gpu

METERS = range(7)
# ratio 4 (192 k -> 48 k, dsp_size 256: 150 blocks) and ratio 2 (dsp_rate 24000, dsp_size 64: 300 blocks), about 0.8 s each
ENGINES = {"ratio4": Case((192000, 48000, 48000, 256), (USB, AM, LSB)), "ratio2": Case((96000, 24000, 24000, 64), (USB, AM, LSB))}


@pytest.fixture(scope="module", params=sorted(ENGINES))
def case(request):
    c = ENGINES[request.param]
    return c, c.inputs()


def _engine(qh, c, form, snba=1):
    e = c.engine(qh, snba)
    e.enable_meters(True)
    e.set_snba_form(form)
    assert e.snba_form() == form
    return e


def _meters(e, nch):
    return [[e.GetRXAMeter(ch, mt) for mt in METERS] for ch in range(nch)]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_the_passes_equal_the_single_kernel_in_every_bit(qh, case):
    c, x = case
    ys, ms = [], []
    for form in (0, 1):
        e = _engine(qh, c, form)
        ys.append(c.through(e, x))
        ms.append(_meters(e, c.nch))
        e.close()
    assert np.all(np.isfinite(ys[0])) and np.abs(ys[0]).max() > 1e-3
    for ch in range(c.nch):
        assert _same_bits(ys[0][ch], ys[1][ch]), (ch, int(np.sum(ys[0][ch] != ys[1][ch])))
    assert np.array_equal(np.array(ms[0]).view(np.uint64), np.array(ms[1]).view(np.uint64))


def test_the_form_may_change_between_calls(qh, case):
    """one state layout for both forms: an engine that alternates them call by call equals one that stays with the single kernel"""
    c, x = case
    a, b = _engine(qh, c, 0), _engine(qh, c, 0)
    ya, yb = [], []
    for k, (lo, hi) in enumerate(c.cuts()):
        b.set_snba_form(k & 1 ^ 1)
        seg = x[:, lo * c.insize:hi * c.insize]
        ya.append(a.process_host(seg)); yb.append(b.process_host(seg))
    assert _same_bits(np.concatenate(ya, axis=1), np.concatenate(yb, axis=1))
    a.close(); b.close()


def test_the_same_with_snb_switched_on_in_mid_stream(qh, case):
    c, x = case
    ys = []
    for form in (0, 1):
        e = _engine(qh, c, form)
        e.SetRXASNBARun(1, 0)
        ys.append(c.through(e, x, {2: lambda t, a, i: t.SetRXASNBARun(*a, 1) if i == 1 else None}))
        ys.append(np.array(_meters(e, c.nch)))
        e.close()
    assert _same_bits(ys[0], ys[2]) and _same_bits(ys[1], ys[3])


def test_the_same_under_graph_replay(qh, case):
    """block-at-a-time calls on fixed device buffers: the replayed three passes equal the plainly launched single kernel"""
    c, x = case
    dev = torch.device("cuda:0")
    nb = min(c.nblk, 150)
    ys, launches = [], []
    for form, replay in ((0, False), (1, True)):
        e = _engine(qh, c, form)
        e.set_graph_replay(replay)
        d_in = torch.zeros((c.nch, c.insize), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((c.nch, c.outsize), dtype=torch.complex128, device=dev)
        y = np.zeros((c.nch, nb * c.outsize), dtype=np.complex128)
        for b in range(nb):
            d_in.copy_(torch.from_numpy(x[:, b * c.insize:(b + 1) * c.insize]))
            torch.cuda.synchronize()
            e.process_ptr(d_in.data_ptr(), c.insize, d_out.data_ptr(), c.outsize, 1)
            e.synchronize()
            y[:, b * c.outsize:(b + 1) * c.outsize] = d_out.cpu().numpy()
        ys.append(y); ys.append(np.array(_meters(e, c.nch))); launches.append(e.graph_launches())
        e.close()
    assert launches[0] == 0 and launches[1] >= nb - 5
    assert np.abs(ys[0]).max() > 1e-3
    assert _same_bits(ys[0], ys[2]) and _same_bits(ys[1], ys[3])
