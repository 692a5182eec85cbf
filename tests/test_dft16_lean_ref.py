"""The 144-operation 16-point butterfly (qh_fft.hpp Dft16Lean) and the radix-2 Dft<16> it replaces in the fp64 4096-point tiles, both
restated in numpy (tests/dft16_lean_ref.py) and held against an exact transform in long double: the 16 unit vectors, the 16
single-bin inputs and 1000 random vectors, forward and inverse.  The two forms compute the same sums in another order, so the new
form's largest error may be at most twice the old form's on the same inputs.  No GPU.

Measured (largest error per part against the exact transform, new / old):
    forward   unit vectors 4.8e-17 / 9.3e-17   single bins 1.02e-15 / 1.70e-15   random 3.20e-15 / 3.23e-15
    inverse   unit vectors 4.8e-17 / 9.3e-17   single bins 1.02e-15 / 1.70e-15   random 3.20e-15 / 3.26e-15
A constant wrong in its 14th digit gives 1.0e-13 on the random vectors, a wrong sign 12.7 (profiles/dft16_lean.md)."""
import numpy as np
import pytest

import dft16_lean_ref as D


@pytest.fixture(scope="module")
def material():
    assert np.finfo(np.longdouble).nmant >= 63, "the exact transform needs a long double with a 64-bit significand"
    xs = D.inputs()
    return {(name, inv): (x, D.dft16_exact(x, inv)) for name, x in xs.items() for inv in (False, True)}


def errors(material, inv, form):
    return {name: D.largest_error(form(x, inv), want) for (name, i), (x, want) in material.items() if i == inv}


def test_exact_transform_is_a_dft(material):
    """The long-double reference against numpy's transform (float64 accuracy), so that a wrong reference cannot pass both forms."""
    for (name, inv), (x, want) in material.items():
        ref = np.fft.ifft(x, axis=-1) * 16 if inv else np.fft.fft(x, axis=-1)
        assert D.largest_error(ref, want) < 1e-13, (name, inv)


@pytest.mark.parametrize("inv", [False, True], ids=["forward", "inverse"])
def test_new_form_within_twice_the_old_forms_error(material, inv):
    new, old = errors(material, inv, D.dft16_lean), errors(material, inv, D.dft16_radix2)
    for name in new:
        print("%s %s: new %.3e old %.3e" % ("inverse" if inv else "forward", name, new[name], old[name]))
    assert max(old.values()) < 64 * 2.0 ** -53 * 16, "the old form itself is off: the restatement is wrong"
    for name in new:                        # each set of inputs on its own, which also holds the largest of all
        assert new[name] <= 2.0 * old[name], name


@pytest.mark.parametrize("inv", [False, True], ids=["forward", "inverse"])
def test_forms_agree_in_natural_order(material, inv):
    """Every output of the new form sits in the old form's place (a permuted output would be an error of the size of a sample)."""
    x, want = material[("random", inv)]
    assert np.max(np.abs(D.dft16_lean(x, inv) - D.dft16_radix2(x, inv))) < 1e-13


@pytest.mark.parametrize("fault", ["constant", "sign"])
def test_a_planted_fault_fails_the_check(material, fault):
    """One constant wrong in its 14th digit, or one sign wrong in one rotation: the check above must fail."""
    old = errors(material, False, D.dft16_radix2)
    bad = errors(material, False, lambda x, inv: D.dft16_lean(x, inv, fault=fault))
    print("fault %s: %s against old %s" % (fault, bad, old))
    assert max(bad.values()) > 2.0 * max(old.values())
    assert bad["random"] > 2.0 * old["random"]
