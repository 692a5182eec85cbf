"""tests/rxa_taps_ref.Siphon (xsiphon mode 0, suck, flush_siphon restated from wdsp/siphon.c) against plain slicing of the stream.

With insize < sipsize the ring holds the stream's newest sipsize samples and suck(n) returns the newest n, zeros where the stream (since
the last flush) is shorter.  With insize >= sipsize every block leaves its last sipsize samples at the ring's start and idx stays 0, so
suck(n) reads backwards from the ring's END: the newest n samples of the last block, whatever n.  No GPU."""
import numpy as np
import pytest

from rxa_taps_ref import SIPSIZE, Siphon

READS = (1, 100, 4096)


def _stream(n, seed=0):
    r = np.random.default_rng(seed)
    return r.standard_normal(n) + 1j * r.standard_normal(n)


def _newest(x, n):
    """the newest n samples of a stream that started from zeros"""
    x = np.concatenate([np.zeros(max(n - x.size, 0), dtype=np.complex128), x])
    return x[x.size - n:]


@pytest.mark.parametrize("insize", [64, 2048])
def test_ring_writes_wrap(insize):
    nblk = 3 * SIPSIZE // insize + 5                        # wraps the ring three times, ends off a multiple of the ring
    x = _stream(nblk * insize, seed=insize)
    s = Siphon(insize)
    for k in range(nblk):
        s.xsiphon(x[k * insize:(k + 1) * insize])
        assert s.idx == ((k + 1) * insize) % SIPSIZE
        for n in READS:
            assert np.array_equal(s.suck(n), _newest(x[:(k + 1) * insize], n)), (k, n)


@pytest.mark.parametrize("insize", [4096, 8192])
def test_long_blocks_leave_idx_alone(insize):
    x = _stream(3 * insize, seed=insize)
    s = Siphon(insize)
    for k in range(3):
        s.xsiphon(x[k * insize:(k + 1) * insize])
        assert s.idx == 0
        assert np.array_equal(s.sipbuff, x[(k + 1) * insize - SIPSIZE:(k + 1) * insize])
        for n in READS:
            assert np.array_equal(s.suck(n), x[(k + 1) * insize - n:(k + 1) * insize]), (k, n)


def test_a_read_before_the_ring_is_full_has_zeros_ahead():
    x = _stream(5 * 256, seed=7)
    s = Siphon(256)
    s.push(x)
    got = s.suck(4096)
    assert not np.any(got[:4096 - x.size]) and np.array_equal(got[4096 - x.size:], x)
    assert np.array_equal(s.suck(100), x[-100:])


def test_push_is_xsiphon_block_by_block():
    x = _stream(17 * 256, seed=9)
    a, b = Siphon(256), Siphon(256)
    a.push(x)
    for k in range(17):
        b.xsiphon(x[k * 256:(k + 1) * 256])
    assert a.idx == b.idx and np.array_equal(a.sipbuff, b.sipbuff)


def test_flush():
    x = _stream(40 * 256, seed=11)
    s = Siphon(256)
    s.push(x[:23 * 256])
    assert s.idx != 0
    s.flush()
    assert s.idx == 0
    for n in READS:
        assert not np.any(s.suck(n))
    s.push(x[23 * 256:])
    for n in READS:
        assert np.array_equal(s.suck(n), _newest(x[23 * 256:], n))
