"""GPU (-m gpu): the memory pipeline of the matrix-function G-layer kernel (csrc/spectral_fused.hip) -- its row sweep and its
assembly read the lower triangle of Z with loads that EVERY lane issues (a lane outside the triangle reads the nearest element
inside and drops it with a select; in the update pass it also writes the diagonal element's new value once more), and the row
sweep works in trips of four rows per wave with the rows left over taken one by one.  What can go wrong with that, and only shows
at particular sizes:

  1. the edges of the clamping and of the trip structure: D below the number of waves, around one and two trips of 2 x 12 rows,
     around the 64-column chunks, at the change of shape (4 / 12 waves) and at the single-lane corner column of n = 257 -- every
     output against the float64 oracle, with the bounds of tests/test_gpu_glayer_route.py, in the three update modes;
  2. a clamped load that leaks into arithmetic, or a select replaced by a multiplication: NaN instead of zeros above the diagonal
     of Z and of the incoming G changes no bit of any result, and nothing above the diagonal or outside the B matrices is written;
  3. run-to-run equality at scale (the border row of E^2 shares its slabs with the restructured phases), and within each run the
     same bits for every copy of a matrix: the 2048 are the trace's five repeated, and a result may not depend on the neighbours.

All through ops.glayer_spectral on caller-supplied state.  The inputs are the per-layer states of an oracle forward (float64) of
B = 5 signals; the seeds (SEEDS: of the weights and of the signals, per size) are chosen so that at every size at least 4 of the
5 matrices are accepted, and REJECTED holds, per case, how many the kernel rejected before its loads were restructured
(profiles/r13/README.md): a case may not reject more.
"""
import ctypes
import functools

import pytest
import torch

from admm_net_amd import _lib, ops, synth
from oracle import admm_net_ref as R
from test_gpu_glayer_route import (S_CORNER_Z, SENT_G, SENT_RN, U32, _bits, _check_accepted, _check_status, _model, _reference,
                                   _tril)

pytestmark = pytest.mark.gpu

B, K, PERTURB = 5, 3, 0.3
DEFAULT_SEEDS = (7, 13)   # (seed of the weights, seed of the signals)
# with the default weights D = 63 has a kink of the eigenvalue map inside every bulk (all five rejected: flag 4), D = 128 and 129
# reject two of five
SEEDS = {63: (2, 13), 128: (2, 13), 129: (2, 13)}
EDGES = (8, 24, 25, 26, 48, 49, 63, 64, 65, 128, 129, 192, 255, 256)
GRIDS = {8: (2, 4), 24: (4, 6), 25: (5, 5), 26: (2, 13), 48: (6, 8), 49: (7, 7), 63: (7, 9), 64: (8, 8), 65: (5, 13),
         100: (10, 10), 128: (8, 16), 129: (3, 43), 192: (12, 16), 255: (15, 17), 256: (16, 16)}   # D -> (Nb, Nd)
MODES = (0, 1, 2)


def _cases(sizes):
    return [pytest.param(D, w, mode, id=f"D{D}-W{w}-mode{mode}") for D in sizes for w in ((12, 4) if D <= 128 else (12,))
            for mode in MODES]


# matrices (of 5) the kernel rejected on these inputs before the change, per (D, waves, mode); absent: none.  (With these seeds it
# rejected none in any of the 72 cases.)
REJECTED = {}

NAN = complex(float("nan"), float("nan"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def _seeds(D, seeds=None):
    return seeds or SEEDS.get(D, DEFAULT_SEEDS)


@functools.lru_cache(maxsize=None)
def _trace(D, seeds):
    Nb, Nd = GRIDS[D]
    torch.set_num_threads(min(4, torch.get_num_threads()))
    sd = R.make_weights(Nb, Nd, K, seed=seeds[0], head=False, perturb=PERTURB)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=seeds[1])
    tr = []
    R.forward(sd, torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s), Nb, Nd, K, dtype="f64", trace=tr)
    return sd, tr


def _inputs(D, mode, seeds=None):
    return _inputs_of(D, mode, _seeds(D, seeds))


@functools.lru_cache(maxsize=None)
def _inputs_of(D, mode, seeds):
    """The call of layer k (2 in modes 0 and 1, 1 in mode 2) and its float64 expectations, computed once and never modified:
    dict(k, phi, h, Z, G, prev, Z_exp, bound, G_ref, rn_ref).  Z, G: the lower triangles count; G is what the kernel finds in
    its output buffer (a sentinel in mode 0, G of layer k - 1 otherwise)."""
    Nb, Nd = GRIDS[D]
    sd, tr = _trace(D, seeds)
    n = D + 1
    k = 1 if mode == 2 else 2
    phi, h = tr[k]["phi"].to(torch.complex64), tr[k]["h"].float()
    if mode == 0:
        Z = tr[k - 1]["Z"].to(torch.complex64)
        G = torch.full((B, n, n), SENT_G, dtype=torch.complex64)
        prev, Z_exp, bound = (None, None, None), Z.to(torch.complex128), None
    else:
        p = tr[k - 1]
        phi_p, h_p, G = p["phi"].to(torch.complex64), p["h"].float(), p["G"].to(torch.complex64)
        alpha = p["arho"].float()
        Z = tr[k - 2]["Z"].to(torch.complex64) if mode == 1 else torch.zeros(B, n, n, dtype=torch.complex64)
        m = _model(sd, Nb, Nd, K)
        W = m.packed_weights(torch.device("cuda:0")).cpu()
        corner_zp = float(W[_lib.load().admmnet_layer_weight_offset(ctypes.byref(m.cfg()), k - 1) + S_CORNER_Z])
        C_p = R.block_matrix(phi_p.to(torch.complex128), h_p.double(), corner_zp)
        a64 = alpha.double().reshape(-1, 1, 1)
        Z_exp = Z.to(torch.complex128) + a64 * (G.to(torch.complex128) - C_p)
        bound = 4 * U32 * (Z.abs().double() + a64.abs() * (G.abs().double() + C_p.abs()))   # (test_gpu_glayer_route: three roundings)
        prev = (alpha, phi_p, h_p)
    G_ref, rn_ref = _reference(sd, k, phi, h, Z_exp)
    return dict(k=k, phi=phi, h=h, Z=Z, G=G, prev=prev, Z_exp=Z_exp, bound=bound, G_ref=G_ref, rn_ref=rn_ref)


def _run(dev, D, waves, mode, Z, G, seeds=None):
    """One call on device copies of Z, G (host tensors [B, n, n]) placed between two poisoned guard matrices; returns the host images
    of the whole allocations (Z, G: [B + 2, n, n]), rn, flag, status."""
    Nb, Nd = GRIDS[D]
    sd, _ = _trace(D, _seeds(D, seeds))
    x = _inputs(D, mode, seeds)
    m = _model(sd, Nb, Nd, K)
    n = D + 1
    Zd = torch.full((B + 2, n, n), NAN, dtype=torch.complex64, device=dev)
    Gd = torch.full((B + 2, n, n), NAN, dtype=torch.complex64, device=dev)
    Zd[1:B + 1] = Z.to(dev)
    Gd[1:B + 1] = G.to(dev)
    rn = torch.full((B,), SENT_RN, device=dev)
    flag, st = ops.glayer_spectral(m, x["k"], x["phi"].to(dev), x["h"].to(dev), Zd[1:B + 1], Gd[1:B + 1], rn, mode, *x["prev"],
                                   waves=waves)
    torch.cuda.synchronize()
    return Zd.cpu(), Gd.cpu(), rn.cpu(), flag.cpu(), st.cpu()


# ------------------------------------------------------------------------------------------------ 1. edges against the oracle
@pytest.mark.parametrize("D,waves,mode", _cases(EDGES))
def test_edges_of_clamping_and_trips_match_the_oracle(dev, D, waves, mode):
    x = _inputs(D, mode)
    tri = _tril(D + 1)
    Zo, G, rn, flag, st = _run(dev, D, waves, mode, x["Z"], x["G"])
    Zo, G = Zo[1:B + 1], G[1:B + 1]
    _check_status(flag, st)
    rejected = int((flag != 0).sum())
    print(f"SFPIPE D={D} W{waves} mode {mode}: flags {flag.tolist()} rejected {rejected}")
    if mode == 0:
        assert torch.equal(_bits(Zo), _bits(x["Z"]))                      # Z is input only
    else:   # the folded update, every matrix (the eigensolver reads the Z of the rejected ones)
        dz = (Zo.to(torch.complex128) - x["Z_exp"]).abs()
        bad = (dz > x["bound"]) & tri
        assert not bad.any(), ("fold", [tuple(i.tolist()) for i in bad.nonzero()[:8]], float((dz - x["bound"])[bad].max()))
    worst = _check_accepted(G, rn, flag, x["G_ref"], x["rn_ref"], tri, f"D={D} W{waves} mode {mode}")
    rej = flag != 0
    assert torch.equal(_bits(G[rej]), _bits(x["G"][rej])) and bool((rn[rej] == SENT_RN).all())
    print(f"SFPIPE D={D} W{waves} mode {mode}: worst G error {worst:.2e}")
    assert rejected <= REJECTED.get((D, waves, mode), 0), (rejected, flag.tolist())
    assert rejected <= 1                                                  # (the seed's promise: 4 of 5 accepted)


# ------------------------------------------------------------------------ 2. nothing outside the lower triangle is read or written
@pytest.mark.parametrize("D,waves,mode", _cases((25, 65, 129, 256)))
def test_nothing_outside_the_lower_triangle_is_read_or_written(dev, D, waves, mode):
    x = _inputs(D, mode)
    n = D + 1
    tri = _tril(n)
    upper = ~tri
    runs = []
    for fill in (complex(0.0, 0.0), NAN):
        Z, G = x["Z"].clone(), x["G"].clone()
        Z[:, upper] = fill
        G[:, upper] = fill
        Zo, Go, rn, flag, _ = _run(dev, D, waves, mode, Z, G)
        # what was poisoned is bit-identical afterwards: the upper triangles and the two guard matrices
        for out, src in ((Zo, Z), (Go, G)):
            assert torch.equal(_bits(out[1:B + 1])[:, upper], _bits(src)[:, upper])
            guard = _bits(torch.full((n, n), NAN, dtype=torch.complex64))
            assert torch.equal(_bits(out[0]), guard) and torch.equal(_bits(out[B + 1]), guard)
        runs.append((Zo[1:B + 1], Go[1:B + 1], rn, flag))
    (Za, Ga, rna, fa), (Zb, Gb, rnb, fb) = runs
    assert torch.equal(fa, fb), (fa.tolist(), fb.tolist())
    assert torch.isfinite(Zb[:, tri]).all() and torch.isfinite(Gb[:, tri]).all()
    assert torch.equal(_bits(Ga)[:, tri], _bits(Gb)[:, tri]) and torch.equal(_bits(rna), _bits(rnb))
    assert torch.equal(_bits(Za)[:, tri], _bits(Zb)[:, tri])
    assert (fa == 0).any()


# ------------------------------------------------------------------------------------------------------ 3. run-to-run equality
@pytest.mark.parametrize("D", [256, 100])
def test_three_runs_give_the_same_bits_at_scale(dev, D):
    """2048 matrices (the five of the trace, repeated), the update folded in (mode 1), the forward's own shape: 12 waves at
    D = 256, 4 at D = 100 with three workgroups per CU.  Within each run item j, a copy of item j - 5, has its bits in Z, G, rn
    and flag."""
    NB = 2048
    x = _inputs(D, 1)
    Nb, Nd = GRIDS[D]
    sd, _ = _trace(D, _seeds(D))
    m = _model(sd, Nb, Nd, K)
    idx = torch.arange(NB, device=dev) % B
    alpha, phi_p, h_p = (t.to(dev)[idx].contiguous() for t in x["prev"])
    phi, h = x["phi"].to(dev)[idx].contiguous(), x["h"].to(dev)[idx].contiguous()
    Z0, G0 = x["Z"].to(dev)[idx].contiguous(), x["G"].to(dev)[idx].contiguous()
    first = None
    for _ in range(3):
        Z, G = Z0.clone(), G0.clone()
        rn = torch.full((NB,), SENT_RN, device=dev)
        flag, st = ops.glayer_spectral(m, x["k"], phi, h, Z, G, rn, 1, alpha, phi_p, h_p)
        torch.cuda.synchronize()
        out = tuple(torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32) for t in (Z, G, rn, flag))
        # within the run: item j holds the problem of item j - B, so it owes the same bits whatever ran beside it (compared
        # directly, as words: NB is no multiple of B)
        for t, name in zip(out, ("Z", "G", "rn", "flag")):
            ne = t[B:] != t[:-B]
            assert not bool(ne.any()), (name, "differs between copies of one matrix", int(ne.sum()),
                                        "first at item %d" % (B + int(ne.reshape(NB - B, -1).any(1).to(torch.uint8).argmax())))
        if first is None:
            first = out
            assert int((flag == 0).sum()) >= NB // 2
        else:
            for a, b, name in zip(first, out, ("Z", "G", "rn", "flag")):
                assert torch.equal(a, b), (name, int((a != b).sum()))
