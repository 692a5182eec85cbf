"""The fp64 4096-point tiles on the 144-operation butterfly (qh_fft.hpp Dft16Lean, FftSplit4096<.., LEAN16>): the band stage on
4096-point tiles with the meters off and on, the front stage at folds 2, 4 and 8, the two-group 8192-point tile and one fp64 FirBank,
every output sample inside the per-sample bound of tests/rxa_linear_ref.py (16 E plus the oscillator's term; reference, model and
margin are that module's), and every engine case equal, bit for bit, to its own run through process_ptr with graph replay on.

Three channels, three equal calls: the second crosses a call seam and both halves of the delay lines, and a replay needs the same
call a third time (a plain call, the capture, the replay); two consecutive calls would do for the bound alone.  Sizes per call:
    band, 4096-point tiles     n_mid = 2 * 2048 + 300 (dsp_size 4): two tiles and a ragged one.  With the meters on the fused taps need
                               dsp_size >= 64, so that case runs 2 * 2048 + 320 = 69 blocks of 64
    two-group 8192-point tile  n_mid = 2 * 6144 + 300
    front, folds 2, 4, 8       two tiles of the fold's Lf outputs and 100 more (nbp0 off: the front is the chain's last stage)
    FirBank, 153 taps          two tiles of 3944 and 300 more
Inputs: the suite's tones ('clean'), and unit impulses at tile positions 0, 1, 16, 17, 255, 256 and 4095 of the first two tiles of
every call -- another lane, register and exchange digit of the transform each (in the front cases the positions are those of the
tile's window up to the stage's phase offset, below the fold).  FirBank has no replay path; it is held to the bound alone.

Measured (profiles/dft16_lean.md): the tones run at 0.19 to 0.40 of the bound (3.5 to 11 E), the impulses at 0.22 to 0.53 (4.5 to
20 E, the largest in the fold-2 front), FirBank at 0.08 and 0.09 of 16 E; every replayed run equals its plain run.  -m gpu."""
import numpy as np
import pytest

import filter_forms_ref as F
import rxa_linear_ref as R

pytestmark = pytest.mark.gpu

POSITIONS = (0, 1, 16, 17, 255, 256, 4095)
NCH = 3


def _calls_of(cs):
    return tuple(int(v) for v in cs.schedule.split(":")[1].split(","))


@pytest.fixture(scope="module", autouse=True)
def own_calls_and_inputs():
    """rxa_linear_ref lays out its calls and inputs by name; this file's cases carry theirs in the name ('calls:a,b,c' blocks per
    call, 'tilepos:P:step' = impulses at POSITIONS of the tiles that start at k step - P input samples of every call) and every other
    name goes to the module's own functions."""
    call_blocks, make_input = R.call_blocks, R.make_input

    def blocks(cs):
        return _calls_of(cs) if cs.schedule.startswith("calls:") else call_blocks(cs)

    def inputs(cs, c):
        if not cs.kind.startswith("tilepos:"):
            return make_input(cs, c)
        P, step = (int(v) for v in cs.kind.split(":")[1:])
        per_in = cs.dsp_size * cs.in_rate // cs.dsp_rate
        x = np.zeros(sum(blocks(cs)) * per_in, dtype=np.complex128)
        start = 0
        for nb in blocks(cs):
            for tile in (0, 1):
                for q, p in enumerate(POSITIONS):
                    i = start + tile * step - P + p
                    if 0 <= i < start + nb * per_in:
                        x[i] += 1j ** ((q + tile + c) % 4)
            start += nb * per_in
        return x

    mp = pytest.MonkeyPatch()
    mp.setattr(R, "call_blocks", blocks)
    mp.setattr(R, "make_input", inputs)
    yield
    mp.undo()


def _front_geometry(in_rate):
    taps, L, M = R.resampler(in_rate, 48000)
    fold, pick, P, Lf, per_tile = F.stage_geometry(taps.size, M)
    assert L == 1 and fold == M and pick == 1
    return P, Lf


def _case(what, kind):
    """(case, set_band_tile's argument, meters) of a run; built inside the test, since the front's geometry needs the oracle's taps."""
    def k(P, step):
        return kind if kind == "clean" else "tilepos:%d:%d" % (P, step)
    name = "%s %s" % (what, kind)
    # the band stage alone behind the pointwise shift (in_rate = dsp_rate): tile windows start at k step - P input samples
    if what == "band 4096":
        return R.case(name, in_rate=48000, dsp_size=4, kind=k(2047, 2049), schedule="calls:1099,1099,1099"), 4096, False
    if what == "band 4096 meters":
        return R.case(name, in_rate=48000, dsp_size=64, kind=k(2048, 2048), schedule="calls:69,69,69"), 4096, True
    if what == "band 8192":
        return R.case(name, in_rate=48000, dsp_size=4, kind=k(2048, 6144), schedule="calls:3147,3147,3147"), 8192, False
    fold = int(what.split()[-1])
    P, Lf = _front_geometry(48000 * fold)
    nb = (2 * Lf + 100 + 3) // 4
    return R.case(name, in_rate=48000 * fold, dsp_size=4, nbp_run=0, kind=k(P, Lf * fold), schedule="calls:%d,%d,%d" % (nb, nb, nb)), 0, False


RUNS = [(what, kind) for kind in ("clean", "tilepos")
        for what in ("band 4096", "band 4096 meters", "band 8192", "front fold 2", "front fold 4", "front fold 8")]


def run_id(run):
    return ("%s %s" % run).replace(" ", "_")


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_inside_the_bound_and_equal_to_its_replay(qh, run):
    cs, form, meters = _case(*run)
    rec = R.case_ref(cs, NCH, form, meters)
    info = {}
    y = R.run_engine(qh, cs, NCH, form, meters, None, info)
    assert y.shape == rec["want"].shape, "output counts differ from the reference's"
    if form:
        assert info["band_tile"] == form
    w = R.margins(y, rec)
    print("%s: worst error %.3g of its bound, %.3g E; %s outputs from a tile start, %s from a call's"
          % (run_id(run), w["ratio"], w["err_over_E"], w["to_seam"], w["to_call"]))
    R.assert_inside(run_id(run), y, rec["want"], rec["bound"], rec["tiles"], rec["calls"])
    info = {}
    yr = R.run_engine(qh, cs, NCH, form, meters, True, info)
    assert info["graph_launches"] >= 1, "the third call did not replay"
    assert yr.tobytes() == y.tobytes(), "the graph-replayed run differs from the plain one"


@pytest.mark.parametrize("kind", ["clean", "tilepos"])
def test_firbank_153_taps_inside_the_bound(qh, kind):
    """osfir_kernel at fold 1 behind the C ABI's FIR bank: 153 taps, Lf = 3944.  Reference: the convolution in long double
    (rxa_linear_ref.conv_ld); E: filter_forms_ref.os_model in complex128 against it; bound 16 E per sample and part."""
    R.require_long_double()
    ntaps = 153
    P, Lf = F.stage_geometry(ntaps, 1)[2:4]
    assert (P, Lf) == (152, 3944)
    sizes = [2 * Lf + 300] * 2
    n = sum(sizes)
    taps = F.forced_taps(ntaps, 153)
    x = np.zeros((NCH, n), dtype=np.complex128)
    t = np.arange(n, dtype=np.float64)
    for c in range(NCH):
        if kind == "clean":
            rng = np.random.default_rng(153 + c)
            x[c] = np.exp(-2j * np.pi * ((0.034375 * (c + 1) * t) % 1.0)) + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        else:
            for start in (0, sizes[0]):
                for tile in (0, 1):
                    for q, p in enumerate(POSITIONS):
                        i = start + tile * Lf - P + p
                        if 0 <= i < n:
                            x[c, i] += 1j ** ((q + tile + c) % 4)
    want = np.stack([R.conv_ld(x[c], taps) for c in range(NCH)])
    E = max(float(max(np.max(np.abs(m.real - w.real)), np.max(np.abs(m.imag - w.imag))))
            for m, w in ((F.os_model(x[c], taps, 1, F.F64), want[c]) for c in range(NCH)))
    assert E > 0.0
    bank = qh.FirBank(NCH, taps, 1, dtype=F.F64)
    y, starts = F.run_calls(bank, x, sizes)
    assert y.shape == want.shape
    calls, tiles = F.fir_seams(ntaps, 1, sizes)
    w = F.worst_sample(y, want, R.MARGIN * E, tiles, calls)
    print("FirBank 153 %s: worst error %.3g of its bound 16 E, E = %.3g" % (kind, w["ratio"], E))
    R.assert_inside("FirBank 153 taps %s" % kind, y, want, R.MARGIN * E, tiles, calls)
