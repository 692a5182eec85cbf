"""Row b1 pinned by reference execution: the reference's own quisk_wdsp.c (compiled in place into oracle/_ref by
`make -C oracle ref`, plain gcc) against the restatement wo_shim_* of oracle/wdsp_oracle.c, bit for bit, on ragged
sample counts.  The reference build's side is stored: tests/golden/ref_build_golden.npz (tests/golden/make_ref_build_golden.py
hands it an oracle WDSP channel's fexchange0 as an integer address, the way Quisk hands over libwdsp's, quisk_wdsp.py:57-67,
quisk_wdsp.c:77-88; the restatement here gets an identically configured channel).  CPU only."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from quisk_amd import synth

RAGGED = [100, 1024, 3000, 5, 0, 2048 * 4 + 17, 1, 1023, 2, 7000]
CLIP32 = 2147483647.0


def _channel(po, in_size, in_rate):
    o = po.WdspChannel(in_size, 256, in_rate, 48000, 48000)
    o.SetRXAShiftRun(1); o.SetRXAShiftFreq(10000.0); o.RXANBPSetRun(1); o.SetRXAMode(1)
    o.RXASetPassband(300.0, 3000.0); o.SetRXAAGCMode(0); o.SetRXAAGCFixed(0.0)
    return o


PARAMS = [(1024, 192000), (64, 48000), (256, 48000)]
REF_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_build_golden.npz")


def _input(in_rate):
    return synth.make_input_numpy(1, sum(RAGGED), fs=float(in_rate))[0] * CLIP32


def ragged_calls(in_size, in_rate):
    """(count, work array) of every ragged call: the input in front, room for four blocks and a few words behind."""
    x, pos = _input(in_rate), 0
    for k in RAGGED:
        a = np.zeros(k + 4 * in_size + 8, dtype=np.complex128); a[:k] = x[pos:pos + k]
        pos += k
        yield k, a


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("in_size,in_rate", PARAMS)
def test_restated_shim_is_bit_identical_to_the_reference_build(oracle, in_size, in_rate):
    gold = np.load(REF_GOLD)
    key = "shim_%d_%d_" % (in_size, in_rate)
    chan_own = _channel(oracle, in_size, in_rate)
    L = oracle.lib()
    calls = []

    def own_fx(pin, pout):
        calls.append(1)
        err = C.c_int(0)
        L.wo_fexchange0(chan_own.h, pin, pout, err)
        return err.value
    own = oracle.OracleWdspShim(own_fx)
    own.set_parameter(in_size=in_size, in_use=1)

    for i, (k, b) in enumerate(ragged_calls(in_size, in_rate)):
        before = len(calls)
        nb = own.fexchange0(b, k)
        assert nb == gold[key + "n"][i], k
        assert len(calls) - before == gold[key + "blocks"][i], k           # the blocks handed to fexchange0 by this call
        assert _sha(b.view(np.float64)) == gold[key + "sha256"][i], k       # every double, the untouched tail included
    assert calls
    # in_use = 0: the ring is reset and the samples pass through untouched (quisk_wdsp.c:33-38)
    own.set_parameter(in_use=0)
    x = _input(in_rate)
    b = x[:77].copy()
    assert own.fexchange0(b, 77) == 77 == gold[key + "passthrough_n"]
    assert np.array_equal(b, x[:77]) and _sha(b.view(np.float64)) == gold[key + "passthrough_sha256"]


def _known_answer_fx(in_size, seen):
    """fexchange0 writing out[i] = in[i] * (0.5 - 0.25j) for the first in_size/4 samples of a block; the blocks it saw go to `seen`."""
    def fx(pin, pout):
        pin, pout = C.cast(pin, C.POINTER(C.c_double)), C.cast(pout, C.POINTER(C.c_double))
        blk = np.array([complex(pin[2 * i], pin[2 * i + 1]) for i in range(in_size)])
        seen.append(blk)
        for i in range(in_size // 4):
            v = blk[i] * (0.5 - 0.25j)
            pout[2 * i], pout[2 * i + 1] = v.real, v.imag
        return 0
    return fx


def _shims(oracle, in_size, ch):
    """(name, fexchange0(buf, n), seen, close) of every shim at hand: the restatement, and the reference build where oracle/_ref holds it."""
    seen = []
    own = oracle.OracleWdspShim(_known_answer_fx(in_size, seen))
    own.set_parameter(in_size=in_size, in_use=1)
    yield "restatement", own.fexchange0, seen, lambda: own.set_parameter(in_use=0)
    ref = oracle.ref_wdsp_shim_lib()
    if ref is not None:
        seen = []
        fx = _known_answer_fx(in_size, seen)
        fx_t = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int))

        def fexchange0(channel, pin, pout, perr):
            perr[0] = fx(pin, pout)
        cb = fx_t(fexchange0)
        oracle.ref_wdsp_set_parameter(ch, in_size=in_size, fexchange0=C.cast(cb, C.c_void_p).value, in_use=1)
        yield "reference", lambda buf, n: ref.wdspFexchange0(ch, buf.ctypes.data, n), seen, lambda: oracle.ref_wdsp_set_parameter(ch, in_use=0)


def test_known_answer_of_the_reference_shim(oracle):
    """The shim alone, with a fexchange0 that writes out[i] = in[i] * (0.5 - 0.25j) for the first in_size/4 samples:
    scaling by CLIP32 both ways, blocks consumed in order, in_size samples reported per block (quisk_wdsp.c:56-66) -- asked of
    the restatement, which the test above holds to the reference build bit for bit, and of that build itself where it is at hand."""
    in_size, ch = 8, 9
    rng = np.random.default_rng(3)
    x = (rng.integers(-2 ** 30, 2 ** 30, 40) + 1j * rng.integers(-2 ** 30, 2 ** 30, 40)).astype(np.complex128)
    for name, fexchange0, seen, close in _shims(oracle, in_size, ch):
        buf = np.zeros(64, dtype=np.complex128); buf[:19] = x[:19]
        n = fexchange0(buf, 19)
        assert n == 16 and len(seen) == 2, name
        assert np.array_equal(np.concatenate(seen), x[:16] / CLIP32), name
        for b in range(2):
            want = (x[8 * b:8 * b + 2] / CLIP32) * (0.5 - 0.25j) * CLIP32
            assert np.array_equal(buf[8 * b:8 * b + 2], want), name
        buf2 = np.zeros(64, dtype=np.complex128); buf2[:5] = x[19:24]
        assert fexchange0(buf2, 5) == 8, name        # 3 carried + 5 new
        assert np.array_equal(seen[2], x[16:24] / CLIP32), name
        close()
