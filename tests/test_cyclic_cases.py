"""CPU: tests/cyclic_cases.py, the sibling comparison the at-occupancy device tests stand on, shown to fail: a stand-in result
in which one word of one sibling is off by one bit (one ulp) must be found and named -- matrix, copy, element, both bit
patterns -- wherever it sits; a sign of zero and a NaN payload count; floats are never compared."""
import numpy as np
import pytest
import torch

import cyclic_cases as C

P, COPIES = 5, 7
B = P * COPIES


def results(dtype, shape=(6, 4), seed=0):
    """A stand-in for a correct device result: P distinct items repeated cyclically to B."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int32:
        base = torch.randint(-2 ** 31, 2 ** 31 - 1, (P,) + shape, generator=g, dtype=torch.int64).to(torch.int32)
    elif dtype == torch.complex64:
        base = torch.complex(torch.randn((P,) + shape, generator=g), torch.randn((P,) + shape, generator=g))
    else:
        base = torch.randn((P,) + shape, generator=g)
    return C.cyclic(base, B).clone()


def plant(t, j, word, mask=1):
    """Flip `mask` in 32-bit word `word` of batch item j, in place (mask 1 on a float: one ulp)."""
    v = torch.view_as_real(t) if t.is_complex() else t
    v.view(torch.int32).reshape(t.shape[0], -1)[j, word] ^= mask


def test_cyclic_repeats_in_order():
    base = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    got = C.cyclic(base, 15)
    assert got.shape == (15, 3) and got.device == base.device
    assert torch.equal(got, base.repeat(3, 1)) and torch.equal(C.cyclic(base, 7), base.repeat(2, 1)[:7])


@pytest.mark.parametrize("dtype", [torch.complex64, torch.float32, torch.int32], ids=["complex64", "float32", "int32"])
def test_untouched_copies_are_equal(dtype):
    d = C.siblings_differ(results(dtype), P)
    assert d.count == 0 and d.batch is None
    assert "equal" in C.describe("x", d)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.float32, torch.int32], ids=["complex64", "float32", "int32"])
def test_one_planted_bit_is_found_and_named_wherever_it_sits(dtype):
    """Every batch item from P on (item P: the first that has a predecessor; the last sibling: no successor) x the first, a
    middle and the last word of the item."""
    t0 = results(dtype)
    per = C.words(t0).shape[1]
    for j in range(P, B):
        for word in (0, per // 2 + 1, per - 1):
            t = t0.clone()
            plant(t, j, word)
            d = C.siblings_differ(t, P)
            last = j >= B - P
            assert d.count == (1 if last else 2), (j, word, d)     # against its predecessor, and its successor against it
            assert (d.batch, d.problem, d.sibling) == (j, j % P, j // P), (j, word, d)
            cplx = dtype == torch.complex64
            assert (d.element, d.part) == ((word // 2, word % 2) if cplx else (word, 0)), (j, word, d)
            assert d.bits ^ d.other_bits == 1
            assert d.other_bits == int(C.words(t0)[j, word]) & 0xFFFFFFFF
            if dtype != torch.int32:   # one ulp: the values are neighbours in float32
                assert d.value != d.other_value
                assert np.nextafter(np.float32(d.other_value), np.float32(d.value)) == np.float32(d.value)
            else:
                assert abs(d.value - d.other_value) == 1


def test_a_change_in_the_first_copy_is_seen_from_its_successor():
    t = results(torch.float32)
    plant(t, 2, 3)
    d = C.siblings_differ(t, P)
    assert d.count == 1 and (d.batch, d.problem, d.sibling, d.element) == (2 + P, 2, 1, 3)


def test_the_stand_in_names_matrix_and_element():
    """The deliberately wrong stand-in: V [B, n, n] complex64 with the imaginary part of V[23, 4, 7] one ulp off."""
    n = 9
    t = results(torch.complex64, shape=(n, n))
    good = t[23, 4, 7].clone()
    plant(t, 23, 2 * (4 * n + 7) + 1)
    d = C.siblings_differ(t, P)
    assert d.count == 2 and (d.batch, d.problem, d.sibling, d.element, d.part) == (23, 3, 4, 4 * n + 7, 1)
    assert np.float32(d.other_value) == np.float32(good.imag) and d.value != d.other_value
    text = C.describe("V", d, shape=(n, n))
    assert "batch item 23" in text and "(4, 7)" in text and "0x%08x" % d.bits in text and "0x%08x" % d.other_bits in text


def test_every_differing_word_is_counted():
    t = results(torch.float32)
    for j, word in ((B - 1, 0), (B - 2, 5), (B - 2, 6), (B - 3, 23)):   # all in the last copy: no successor counts twice
        plant(t, j, word, mask=0x40)
    d = C.siblings_differ(t, P)
    assert d.count == 4 and (d.batch, d.element) == (B - 3, 23)


def test_the_sign_of_zero_counts():
    t = C.cyclic(torch.zeros(P, 4), B).clone()
    assert C.siblings_differ(t, P).count == 0
    t[B - 1, 2] = -0.0
    assert bool((t[B - 1] == t[B - 1 - P]).all())                         # a float comparison sees nothing
    d = C.siblings_differ(t, P)
    assert d.count == 1 and (d.batch, d.element, d.bits, d.other_bits) == (B - 1, 2, 0x80000000, 0)


def test_nan_payloads_count_and_equal_nans_do_not():
    nan_a = torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.float32)
    nan_b = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    t = C.cyclic(torch.randn(P, 4, generator=torch.Generator().manual_seed(1)), B).clone()
    t[1::P, 3] = nan_a                                                    # every copy of problem 1 holds the same NaN
    assert not bool((t[1 + P] == t[1]).all())                             # a float comparison calls them different
    assert C.siblings_differ(t, P).count == 0
    t[1 + 3 * P, 3] = nan_b
    d = C.siblings_differ(t, P)
    assert d.count == 2 and (d.batch, d.element, d.bits, d.other_bits) == (1 + 3 * P, 3, 0x7FC00001, 0x7FC00000)
    assert np.isnan(d.value) and np.isnan(d.other_value)
    z = torch.complex(t, t.flip(1))                                       # and in a complex tensor, either part
    assert C.siblings_differ(z, P).count == 4


def test_a_ragged_batch_is_refused():
    t = results(torch.float32)
    for bad in (t[:B - 1], t[:P + 1], t[:P - 1]):
        with pytest.raises(ValueError, match="multiple"):
            C.siblings_differ(bad, P)
    assert C.siblings_differ(t[:P], P).count == 0                         # one copy: nothing to compare, nothing differs
    with pytest.raises(ValueError):
        C.siblings_differ(t, 0)


def test_other_dtypes_are_refused():
    with pytest.raises(TypeError):
        C.siblings_differ(torch.zeros(10, 3, dtype=torch.float64), 5)
    with pytest.raises(TypeError):
        C.siblings_differ(torch.zeros(10, 3, dtype=torch.complex128), 5)

