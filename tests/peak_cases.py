"""The shared table of the peak-search tests (tests/test_peak_cases_host.py on the CPU, tests/test_gpu_peak_cases.py on the
device): designed spectra, the option sets that reach every branch of the refinement, the regional-maxima images, the counters
of what a case reaches, the tie rule, and one search engine that takes its spectrum, its maxima and -- for the host test that
shows the table rejects mistakes -- one deliberate mistake.  Imports nothing that needs a GPU.

A signal is  phi = sum_l a_l kron(s(f_l), conj d(tau_l)) + noise (randn + j randn), evaluated in float64 and cast to
complex64 (what the device reads); s has ybase entries, d has xbase, so |phi^H kron(s(f), conj d(tau))|^2 peaks at (tau_l, f_l).

THE TIE RULE.  A decision of the search is a comparison of two spectrum values: a coarse pixel against an 8-neighbour of a
different value (the regional maxima), or a local arg-max against its runner-up (a refinement round).  Its margin is the
difference of the two in the oracle's float64 image.  The spectrum is |z|^2, z a sum of D = xbase ybase terms phi_k e^{j..}
accumulated separably (depth xbase + ybase); with |z| <= S = sum_k |phi_k| two correct float64 evaluations differ by at most
about (xbase + ybase + c) u S^2, u = 2^-53.  EPS takes c = 16 and a factor 64 for the sincos arguments (2 pi k x, |arg| up to
about 2 pi base) and the final square:  eps = 64 (xbase + ybase + 16) 2^-53 S^2.  A decision whose margin is below eps is a
numerical tie: it would be left out of a comparison.  The table is built so that NO decision of any case is a tie
(test_peak_cases_host.py asserts it), so the device tests compare everything.  On an axis whose base is 1 the spectrum is
exactly constant by construction (d = [1]); equal values along that axis are no decisions, and what is compared there is the
plateau handling and the first-arg-max rule."""
import functools

import numpy as np

from oracle import peak_search_ref as PO

NOISE = 0.05
SEEDS = (2, 10)     # chosen with the oracle among 1 .. 10: the two whose smallest margin (case deep, round 5) is largest, > 2000 eps
_STEPS65 = dict(xstep=1 / 24, ystep=1 / 20)


def _case(xbase, ybase, tones, **opts):
    return dict(xbase=xbase, ybase=ybase, tones=tuple(tones), opts=opts)


CASES = {
    "corner": _case(6, 5, [(0.0, -0.5), (0.4, 0.1)], **_STEPS65, iter=3),
    "high_edge_rf0.9": _case(6, 5, [(0.97, 0.47), (0.3, -0.2)], **_STEPS65, reducefactor=0.9, iter=4),
    "high_edge_rf1.0": _case(6, 5, [(0.97, 0.47), (0.3, -0.2)], **_STEPS65, reducefactor=1.0, iter=2),
    "high_edge_rf2.0": _case(6, 5, [(0.97, 0.47), (0.3, -0.2)], **_STEPS65, reducefactor=2.0, iter=2),
    "custom_range": _case(7, 4, [(0.35, 0.05), (0.6, 0.2)], xmin=0.2, xmax=0.7, ymin=-0.25, ymax=0.3, xstep=0.03,
                          ystep=0.04, reducefactor=0.25, iter=2),
    # ay = arange(ymin, ymax - XSTEP, ystep): a 1 x 19 image; round 1 is skipped (ly = 1.5), rounds 2 and 3 run
    "skipped_round": _case(6, 5, [(0.3, -0.5), (0.7, -0.5)], xstep=0.05, ystep=5.0, reducefactor=0.3, iter=3),
    # xmax - lx < xmin in every round: no round runs, every height stays 0.0 although iter > 0
    "no_round_runs": _case(6, 5, [(0.5, 0.0)], xmin=0.4, xmax=0.6, xstep=0.05, ystep=0.05, reducefactor=5, iter=2),
    # round 1 runs (lx = 0.12), round 2 is skipped (lx = 0.48 >= xmax - xmin - ..): the height of round 1 must survive
    "late_skip": _case(7, 4, [(0.35, 0.05), (0.6, 0.2)], xmin=0.2, xmax=0.7, ymin=-0.25, ymax=0.3, xstep=0.03,
                       ystep=0.04, reducefactor=4, iter=2),
    "xbase17": _case(17, 3, [(0.21, -0.3), (0.8, 0.25)], xstep=1 / 68, ystep=1 / 12, iter=2),     # nx = 67
    "xbase16": _case(16, 3, [(0.21, -0.3), (0.8, 0.25)], xstep=1 / 64, ystep=1 / 12, iter=2),
    "base1_x": _case(1, 12, [(0.0, 0.13)], xstep=0.1, ystep=1 / 48, iter=2),
    "base1_y": _case(12, 1, [(0.13, 0.0)], xstep=1 / 48, ystep=0.1, iter=2),
    "tiny_2x2": _case(2, 2, [(0.3, 0.2)], xstep=1 / 8, ystep=1 / 8),
    "tiny_1x1": _case(1, 1, [(0.3, 0.2)], xstep=1 / 8, ystep=1 / 8),
    "deep": _case(6, 5, [(0.31, 0.12), (0.77, -0.33)], **_STEPS65, iter=5),
    # noise alone: more than 256 maxima, the tile of estimate.hip and the default capacity of the list.  (The number of maxima
    # follows the number of resolution cells, not of pixels: 16 x 16 on 48 x 48 has about 110, 32 x 32 on 96 x 96 over 400.)
    "many_maxima": _case(32, 32, [], xstep=1 / 96, ystep=1 / 96),
}
BASE1 = ("base1_x", "base1_y", "tiny_1x1")


def steer(x, base):
    """utils/mathUtils.py:4-21 as a flat vector."""
    return np.exp(1j * 2 * np.pi * np.linspace(0, (base - 1) * x, base))


def make_phi(xbase, ybase, tones, seed, noise=NOISE):
    """[ybase * xbase] complex64; tone l has amplitude 1 / (1 + l / 2) and phase 0.7 l."""
    rng = np.random.default_rng(seed)
    phi = np.zeros(xbase * ybase, dtype=np.complex128)
    for l, (tau, f) in enumerate(tones):
        phi += np.exp(0.7j * l) / (1 + 0.5 * l) * np.kron(steer(f, ybase), np.conj(steer(tau, xbase)))
    phi += noise * (rng.standard_normal(phi.size) + 1j * rng.standard_normal(phi.size))
    return phi.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def phi_of(name, seed):
    c = CASES[name]
    phi = make_phi(c["xbase"], c["ybase"], c["tones"], seed)
    phi.setflags(write=False)
    return phi


def batch_of(name):
    """[len(SEEDS), D] complex64: both seeds of a case stacked."""
    return np.stack([phi_of(name, s) for s in SEEDS])


def eps_of(phi, xbase, ybase):
    S = float(np.abs(np.asarray(phi, dtype=np.complex128)).sum())
    return 64 * (xbase + ybase + 16) * 2.0 ** -53 * S * S


# ------------------------------------------------------------------------------------------------ the search engine
def literal_spectrum(phi, xs, xbase, ys, ybase):
    X, Y = np.meshgrid(xs, ys)
    return PO.peak_search(np.asarray(phi).astype(np.complex128), X, xbase, Y, ybase)


class Trace:
    """What a search reached: counters per window evaluation (one peak in one round) and the smallest margins."""

    def __init__(self, eps, const_x, const_y):
        self.eps, self.const_x, self.const_y = eps, const_x, const_y
        self.upper = self.lower = self.skipped = self.ran = self.late_skips = 0
        self.shapes = set()            # (ny, nx) of the local grids met
        self.decisions = self.tied = 0
        self.min_margin = np.inf
        self.min_where = None
        self.maxima = 0
        self.coarse = None

    def _decide(self, margin, where):
        self.decisions += 1
        if margin < self.eps:
            self.tied += 1
        if margin < self.min_margin:
            self.min_margin, self.min_where = float(margin), where

    def coarse_image(self, Z):
        self.coarse = Z
        ny, nx = Z.shape
        if self.const_x and self.const_y:
            return                     # 1 x 1: the whole image is one value
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if (dr, dc) == (0, 0):
                    continue
                if (self.const_x and dr == 0) or (self.const_y and dc == 0):
                    continue           # a step along an exactly constant axis: no decision
                a = Z[max(0, dr):ny + min(0, dr), max(0, dc):nx + min(0, dc)]
                b = Z[max(0, -dr):ny + min(0, -dr), max(0, -dc):nx + min(0, -dc)]
                if a.size:      # (equal values off a constant axis count as a margin of 0: a tie)
                    m = np.abs(a - b)
                    self.decisions += m.size
                    self.tied += int((m < self.eps).sum())
                    if m.min() < self.min_margin:
                        self.min_margin, self.min_where = float(m.min()), "coarse"

    def local_image(self, LZ, rnd):
        self.shapes.add(LZ.shape)
        if self.const_x:
            assert (LZ == LZ[:, :1]).all()
            LZ = LZ[:, :1]
        if self.const_y:
            assert (LZ == LZ[:1, :]).all()
            LZ = LZ[:1, :]
        if LZ.size > 1:
            v = np.sort(LZ.ravel())
            self._decide(v[-1] - v[-2], f"round {rnd}")


MISTAKES = ("ay_minus_ystep", "upper_clip_at_max", "step_kept_by_skipped_round", "height_reset_by_skipped_round",
            "floor_for_ceil", "points_start_plus_i_step", "last_argmax", "reshape_xbase_ybase", "min_exchanged",
            "reducefactor_once")


def search(phi, xbase, ybase, opts=None, spectrum=literal_spectrum, maxima=PO.regional_maxima_floodfill, mistake=None,
           trace=None):
    """peakSearchUtils.py:63-173 with per-peak state, the way the device runs it, so that one ``mistake`` of MISTAKES can be
    switched on.  With mistake = None it returns
    the bits of oracle.peak_search_ref.alt_peak_search_literal (asserted by the host test)."""
    assert mistake is None or mistake in MISTAKES
    so = {'xmin': 0, 'xmax': 1, 'xstep': 0.01, 'ymin': -0.5, 'ymax': 0.5, 'ystep': 0.01, 'reducefactor': 0.1, 'iter': 1}
    so.update(opts or {})
    xmin, xmax, xstep = so['xmin'], so['xmax'], so['xstep']
    ymin, ymax, ystep = so['ymin'], so['ymax'], so['ystep']
    rf, iters = so['reducefactor'], so['iter']
    if mistake == "min_exchanged":
        xmin, ymin = ymin, xmin
    if mistake == "reshape_xbase_ybase":
        inner = spectrum

        def spectrum(p, xs, xb, ys, yb):
            return inner(np.asarray(p).reshape(xb, yb).T.reshape(-1), xs, xb, ys, yb)
    ax = np.arange(xmin, xmax - xstep, xstep)
    ay = np.arange(ymin, ymax - (ystep if mistake == "ay_minus_ystep" else xstep), ystep)
    if len(ax) == 0 or len(ay) == 0:
        return np.zeros((0, 3))
    Z = spectrum(phi, ax, xbase, ay, ybase)
    if trace:
        trace.coarse_image(Z)
    rows, cols = np.where(maxima(Z))
    num = len(rows)
    if trace:
        trace.maxima = num
    res = np.zeros((num, 3))
    res[:, 0], res[:, 1] = ax[cols], ay[rows]

    def arange(start, stop, step):
        if mistake not in ("floor_for_ceil", "points_start_plus_i_step"):
            return np.arange(start, stop, step)
        q = (stop - start) / step
        n = int(np.floor(q) if mistake == "floor_for_ceil" else np.ceil(q))
        if n <= 0:
            return np.zeros(0)
        i = np.arange(n, dtype=np.float64)
        return start + i * (step if mistake == "points_start_plus_i_step" else (start + step) - start)

    for k in range(num):
        lx, ly = xstep, ystep
        ran_before = False
        for rnd in range(1, iters + 1):
            keep = (lx, ly)
            lx, ly = (rf * xstep, rf * ystep) if mistake == "reducefactor_once" else (rf * lx, rf * ly)
            px, py = res[k, 0], res[k, 1]
            up_x, up_y = (xmax, ymax) if mistake == "upper_clip_at_max" else (xmax - lx, ymax - ly)
            x0, x1 = max(xmin, px - lx), min(up_x, px + lx)
            y0, y1 = max(ymin, py - ly), min(up_y, py + ly)
            lxs, lys = (arange(x0, x1, lx), arange(y0, y1, ly)) if x0 < x1 and y0 < y1 else (np.zeros(0),) * 2
            if len(lxs) == 0 or len(lys) == 0:
                if trace:
                    trace.skipped += 1
                    trace.late_skips += ran_before
                if mistake == "step_kept_by_skipped_round":
                    lx, ly = keep
                if mistake == "height_reset_by_skipped_round":
                    res[k, 2] = 0.0
                continue
            LZ = spectrum(phi, lxs, xbase, lys, ybase)
            if trace:
                trace.ran += 1
                trace.upper += bool(up_x < px + lx or up_y < py + ly)
                trace.lower += bool(xmin > px - lx or ymin > py - ly)
                trace.local_image(LZ, rnd)
            ran_before = True
            m = np.max(LZ)
            pr, pc = np.where(LZ == m)
            pick = -1 if mistake == "last_argmax" else 0
            res[k] = lxs[pc[pick]], lys[pr[pick]], m
    return res


@functools.lru_cache(maxsize=None)
def oracle_of(name, seed):
    """(rows [num, 3], Trace) of one case and seed through the literal spectrum and the flood fill, computed once."""
    c = CASES[name]
    phi = phi_of(name, seed)
    tr = Trace(eps_of(phi, c["xbase"], c["ybase"]), c["xbase"] == 1, c["ybase"] == 1)
    rows = search(phi, c["xbase"], c["ybase"], c["opts"], trace=tr)
    rows.setflags(write=False)
    return rows, tr


def ranking_ties(rows, eps):
    """The ranks (positions in top_rows order) whose order is a numerical tie: neighbours in the sorted list whose heights
    differ, but by less than eps.  Heights of the same bits are no tie: the list order decides, on the device as in top_rows.
    One pair exists in the table: with reducefactor = 2 the windows grow, and two coarse maxima of high_edge_rf2.0 refine to
    the same point up to the last bits of its coordinates.  peak_top's order of such a pair is compared with the oracle's up
    to an exchange; everything else of the pair (both rows, their heights) is compared as usual."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    h = rows[np.argsort(-rows[:, 2], kind="stable"), 2]
    gaps = h[:-1] - h[1:]
    first = np.flatnonzero((gaps > 0) & (gaps < eps))
    return sorted(set(first) | set(first + 1))


# ------------------------------------------------------------------------------------------------ selection stand-ins
def top_rows_reversed_ties(rows, top):
    """top_rows with the order among equal heights reversed (an ascending stable sort, flipped)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    return rows[np.argsort(rows[:, 2], kind="stable")[::-1]][:top]


# ------------------------------------------------------------------------------------------------ regional-maxima images
PLATEAU, HEAD = 5.0, 6.0


def snake(ny, nx, head):
    """A serpentine plateau: even rows at 5.0, joined at alternating ends through the odd rows, 0 elsewhere.  With
    ``head`` its first pixel is 6.0: the plateau has a higher neighbour at one end and must die as a whole, the
    rejection walking its whole length one pixel per pass."""
    img = np.zeros((ny, nx))
    img[0::2] = PLATEAU
    for r in range(1, ny - 1, 2):
        img[r, nx - 1 if (r // 2) % 2 == 0 else 0] = PLATEAU
    if head:
        img[0, 0] = HEAD
    return img


def spiral(n, head):
    """A one-pixel-wide square spiral of 5.0 from the corner inwards, arms two pixels apart (never 8-connected)."""
    img = np.zeros((n, n))
    r = c = 0
    dr, dc = 0, 1
    img[0, 0] = PLATEAU

    def free(a, b):
        return not (0 <= a < n and 0 <= b < n) or img[a, b] == 0

    while True:
        for _ in range(2):
            a, b = r + dr, c + dc
            if 0 <= a < n and 0 <= b < n and img[a, b] == 0 and free(a + dr, b + dc):
                break
            dr, dc = dc, -dr
        else:
            break
        # a turn must not touch the arm it came along: both side cells of the new pixel's far side stay free
        r, c = a, b
        img[r, c] = PLATEAU
    if head:
        img[0, 0] = HEAD
    return img


def checkerboard(ny, nx):
    r, c = np.indices((ny, nx))
    return np.where((r + c) % 2 == 0, 3.0, 2.0)


def border_plateau(ny, nx):
    """A frame of 4.0 touching all four borders around a lower interior with one higher pixel inside."""
    img = np.full((ny, nx), 1.0)
    img[0, :] = img[-1, :] = img[:, 0] = img[:, -1] = 4.0
    img[ny // 2, nx // 2] = 2.0
    return img


BIG = (107, 108)          # the largest image peaks_lds_bytes admits with max_peaks = npix
REFUSED = (108, 108)      # the first one it refuses


def lds_bytes(npix, D=1, max_peaks=None):
    """peaks_lds_bytes of csrc/peaks.hip (PK_THREADS = 256); the limit is 160 KiB."""
    max_peaks = npix if max_peaks is None else max_peaks
    return 8 * npix + 16 * D + 4 * (max_peaks + 257) + 2 * npix + 16


@functools.lru_cache(maxsize=None)
def images():
    """name -> (image, number of maxima the flood fill finds).  The counts of the designed images are known by
    construction and asserted by the host test against the flood fill."""
    rng = np.random.default_rng(5)
    line = np.array([1.0, 3.0, 3.0, 2.0, 5.0, 5.0, 5.0, 1.0, 4.0, 4.0, 6.0, 2.0, 2.0])
    out = {
        "snake_9x11": snake(9, 11, False), "snake_9x11_head": snake(9, 11, True),
        "snake_big": snake(*BIG, False), "snake_big_head": snake(*BIG, True),
        "spiral_21": spiral(21, False), "spiral_21_head": spiral(21, True),
        "checkerboard_7x9": checkerboard(7, 9), "checkerboard_1x2": checkerboard(1, 2),
        "row_1x13": line[None, :].copy(), "column_13x1": line[:, None].copy(), "single_1x1": np.array([[2.0]]),
        "border_plateau_6x8": border_plateau(6, 8),
        "diagonal_step": np.array([[5.0, 0.0, 0.0], [0.0, 6.0, 0.0], [0.0, 0.0, 0.0]]),
        "levels_23x19": rng.integers(0, 3, size=(23, 19)).astype(np.float64),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def image_mask(name):
    m = PO.regional_maxima_floodfill(images()[name])
    m.setflags(write=False)
    return m


def maxima_by_passes(img, connectivity=8, passes=None, spread=True):
    """The device's algorithm (pk_maxima): candidates = no larger neighbour, then rejection spreads over equal
    neighbours one pixel per pass until nothing changes.  Returns (mask, passes that changed something).  The
    stand-ins of the host test: connectivity = 4, passes = a fixed number, spread = False."""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape
    if np.all(img == img.flat[0]):
        return np.zeros((H, W), dtype=bool), 0
    pad = np.full((H + 2, W + 2), -np.inf)
    pad[1:-1, 1:-1] = img
    shifts = [(a, b) for a in (0, 1, 2) for b in (0, 1, 2) if (a, b) != (1, 1) and (connectivity == 8 or a == 1 or b == 1)]
    nb = [pad[a:a + H, b:b + W] for a, b in shifts]
    cand = np.ones((H, W), dtype=bool)
    for v in nb:
        cand &= img >= v
    same = [v == img for v in nb]
    done = 0
    while spread and (passes is None or done < passes):
        cpad = np.ones((H + 2, W + 2), dtype=bool)
        cpad[1:-1, 1:-1] = cand
        kill = np.zeros((H, W), dtype=bool)
        for (a, b), s in zip(shifts, same):
            kill |= s & ~cpad[a:a + H, b:b + W]
        new = cand & ~kill
        if np.array_equal(new, cand):
            break
        cand = new
        done += 1
    return cand, done
