"""The restatement of WDSP's diversity combiner (tests/wdsp_div_ref.py, wdsp/div.c:31-95) against the cases that can be worked by hand:
what the GPU tests compare to has to be right before they mean anything.  No GPU."""
import numpy as np

from wdsp_div_ref import Div, mix

U64 = np.uint64


def _bits(z):
    return np.ascontiguousarray(z, dtype=np.complex128).view(U64)


def test_the_worked_case_with_out_apart_and_laid_over_each_receiver():
    rows = np.array([[1 + 2j], [4 + 8j]])
    ir, qr = [1.0, 0.5], [0.0, -0.25]
    # apart: (1, 2) + (0.5 - 0.25j)(4 + 8j) = (1, 2) + (4, 3)
    assert mix(1, 2, 2, ir, qr, rows)[0] == 5 + 5j
    # out is in1: its samples are zeroed; S = (1, 2), then S + (0.5 - 0.25j) S = (1, 2) + (1, 0.75)
    assert mix(1, 2, 2, ir, qr, rows, onto=1)[0] == 2 + 2.75j
    # out is in0: S = 0 + 1 * 0, then + (4, 3)
    assert mix(1, 2, 2, ir, qr, rows, onto=0)[0] == 4 + 3j


def test_every_operation_is_rounded_on_its_own():
    """nr = 1, Irotate = I = 1 + 2^-30, Qrotate = Q = 1: I I = 1 + 2^-29 + 2^-60 rounds to 1 + 2^-29, and minus 1 that is 2^-29 exactly; a
    fused multiply-add would keep the 2^-60."""
    v = 1.0 + 2.0 ** -30
    y = mix(1, 1, 1, [v], [1.0], np.array([[v + 1j]]))
    assert y[0].real == 2.0 ** -29
    assert y[0].real != 2.0 ** -29 + 2.0 ** -60
    assert y[0].imag == v + v


def test_zeros_in_with_a_negative_rotate_give_plus_zero():
    y = mix(1, 2, 2, [-1.0, -1.0], [-1.0, -1.0], np.zeros((2, 5), dtype=np.complex128))
    assert not _bits(y).any()                           # (-0.0 would show as the sign bit)


def test_defaults_after_create_copy_receiver_zero():
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((3, 7)) + 1j * rng.standard_normal((3, 7))
    d = Div(1, 3)
    assert d.output == 0 and not d.Irotate.any() and not d.Qrotate.any()
    out = np.zeros(7, dtype=np.complex128)
    d.xdiv([r.copy() for r in rows], out)
    assert np.array_equal(_bits(out), _bits(rows[0]))
    d.SetOutput(2)
    d.xdiv([r.copy() for r in rows], out)
    assert np.array_equal(_bits(out), _bits(rows[2]))
    ins = [r.copy() for r in rows]                      # out is in[output]: nothing is done
    d.xdiv(ins, ins[2])
    assert np.array_equal(_bits(ins[2]), _bits(rows[2]))


def test_run_zero_copies_receiver_zero_whatever_output_says():
    rng = np.random.default_rng(2)
    rows = rng.standard_normal((2, 9)) + 1j * rng.standard_normal((2, 9))
    y = mix(0, 2, 2, [1.0, 1.0], [0.0, 0.0], rows)
    assert np.array_equal(_bits(y), _bits(rows[0]))
    y = mix(0, 2, 1, [1.0, 1.0], [0.0, 0.0], rows)
    assert np.array_equal(_bits(y), _bits(rows[0]))


def test_mixing_before_any_rotate_is_set_gives_zeros():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((2, 9)) + 1j * rng.standard_normal((2, 9))
    d = Div(1, 2)
    d.SetOutput(2)
    out = np.full(9, np.nan + 1j * np.nan)
    d.xdiv([r.copy() for r in rows], out)
    assert not _bits(out).any()


def test_set_rotate_copies_the_calls_own_count():
    d = Div(1, 2)
    d.SetRotate(3, [1.0, 2.0, 3.0, 9.0], [4.0, 5.0, 6.0, 9.0])
    assert d.Irotate.tolist() == [1, 2, 3, 0, 0, 0, 0, 0] and d.Qrotate.tolist() == [4, 5, 6, 0, 0, 0, 0, 0]
    d.SetRotate(1, [7.0], [8.0])
    assert d.Irotate.tolist()[:3] == [7, 2, 3] and d.Qrotate.tolist()[:3] == [8, 5, 6]
