"""Cyclic batches (helper of tests/test_cyclic_cases.py and the at-occupancy device tests; no test in it): P distinct problems
repeated to B = P c items and run in one device-filling call.  Every per-matrix kernel owes all c siblings of a problem the same
bits -- a condition, not a tolerance -- and the float64 reference of the P problems is the reference of all B results.

The comparison is on the int32 view of the results, on the tensor's own device: floats are never compared (NaN != NaN would
report equal payloads as different, -0.0 == 0.0 would hide a sign bit)."""
from collections import namedtuple

import torch

# count: differing 32-bit words over all siblings (0: every sibling has the bits of its predecessor, hence of the first);
# the rest describes the first differing word in memory order: batch item, its problem (batch % P), which copy that is (batch // P),
# the element inside the item (flat index in the item's own dtype), the part of it (0; 1 for the imaginary word of a complex
# element), the two bit patterns (unsigned) and the two values (`other`: the same word of item batch - P)
Difference = namedtuple("Difference", "count batch problem sibling element part bits other_bits value other_value")


def cyclic(t, B):
    """t[arange(B) % P] for t of P items, on t's device."""
    P = t.shape[0]
    return t[torch.arange(B, device=t.device) % P]


def words(t):
    """The int32 view [B, words per item] of a complex64, float32 or int32 tensor of B items."""
    if t.dtype == torch.complex64:
        t = torch.view_as_real(t.contiguous())
    elif t.dtype not in (torch.float32, torch.int32):
        raise TypeError("siblings are compared as 32-bit words: complex64, float32 or int32, got %s" % t.dtype)
    return t.contiguous().view(torch.int32).reshape(t.shape[0], -1)


def siblings_differ(t, P):
    """Item j against item j - P for every j >= P, as 32-bit words.  Returns a Difference; .count == 0 says the c copies of
    each of the P problems are bit-identical."""
    B = t.shape[0]
    if P < 1 or B < P or B % P:
        raise ValueError("a cyclic batch holds a whole number of copies: B = %d is no multiple of P = %d" % (B, P))
    v = words(t)
    ne = v[P:] != v[:-P]
    count = int(ne.sum())
    if count == 0:
        return Difference(0, None, None, None, None, None, None, None, None, None)
    per = v.shape[1]
    flat = int(ne.reshape(-1).to(torch.uint8).argmax())   # (the first maximum: the first differing word)
    j, word = P + flat // per, flat % per
    cplx = t.dtype == torch.complex64
    element, part = (word // 2, word % 2) if cplx else (word, 0)
    a, b = int(v[j, word]), int(v[j - P, word])
    scalar = torch.int32 if t.dtype == torch.int32 else torch.float32
    va, vb = (torch.tensor([x], dtype=torch.int32).view(scalar).item() for x in (a, b))
    return Difference(count, j, j % P, j // P, element, part, a & 0xFFFFFFFF, b & 0xFFFFFFFF, va, vb)


def describe(what, d, shape=None):
    """One line for an assertion message; with the item's shape the element as an index tuple."""
    if d.count == 0:
        return "%s: siblings equal" % (what,)
    at = d.element
    if shape:
        idx, rest = [], d.element
        for s in reversed(shape):
            idx.append(rest % s)
            rest //= s
        at = tuple(reversed(idx))
    return ("%s: %d words differ between siblings; first: batch item %d (copy %d of problem %d) element %s part %d: "
            "0x%08x (%r) against 0x%08x (%r) one copy earlier" %
            (what, d.count, d.batch, d.sibling, d.problem, at, d.part, d.bits, d.value, d.other_bits, d.other_value))
