"""The decimating two-transform FFT tile at every long length and run-time radix: the routing restated, and the case table
(no test functions; CPU only).  tests/test_decim_cases.py holds both to the library's plans (rcfm_fft_describe,
rcfm_fft_describe_plan) and to the kernel tables of the headers; tests/test_hip_decim_lengths.py runs the table on the
device.  Stations, truth, mutants and the bound are length_cases' (bound() below: with the one mutant that breaks the
rule the tile restates); the per-case conditioning test of tests/test_length_cases.py runs over CASES below as well.

The routing (route() below), from demod.hip, fused_passes.hip, fft_kernel.h and fft_decim_rt.h:
    plan of B          rcfm_fft_describe(B) = (n1, L) in two passes; the tile sits between FFT_B's last pass (L points) and
                       IFFT_A's first (L2 = A / n1 points)
    decim_plan         A < B, A even, A % (2 n1) == 0, A / n1 >= 16, and rcfm_fft_describe_plan(A, (A / n1, n1)) succeeds
    alloc()'s swap     where (n1, L) does not take the tile and (L, n1) does, B runs as (L, n1)
    the kernels        k_fft_tile2_decim for the instantiated (L, L2) pairs; else k_fft_tile2_decim_rt: L in its list, L2
                       even, 16 <= L2 < L, every radix of the short plan in RT_RADICES -- and what both ask of the two
                       passes (same lines, rows pass into strided pass)
    MFM                only with A % 4 == 0 (run_real); WBFM only behind a two-transform tile of the pilot stage, i.e. with
                       n1 a specialised length (run_wbfm_engine: `paired`)
The short plan's radices are read from rcfm_fft_describe_plan, never assumed: 120 = 12 x 10, 160 = 16 x 10, 192 = 16 x 12 and
256 = 16 x 16 are specialised lists, 90 = 10 x 3 x 3 and 54 = 6 x 3 x 3 the planner's generic choice.
"""

import collections

import fft_model
import length_cases as lc

# fft_decim_rt.h, RCFM_FFT_DECIM_RT_LENGTHS: long length -> its radices (tests/test_decim_cases.py reads the header)
RT_LENGTHS = {100: (10, 10), 120: (12, 10), 125: (5, 5, 5), 128: (8, 8, 2), 150: (15, 10), 160: (16, 10), 192: (16, 12),
              200: (20, 10), 240: (24, 10), 250: (25, 10), 256: (16, 16), 300: (20, 15), 320: (10, 8, 4), 375: (5, 5, 5, 3),
              384: (8, 8, 6), 400: (20, 20), 480: (24, 20), 500: (25, 20), 512: (8, 8, 8)}
RT_RADICES = (2, 3, 4, 5, 6, 8, 10, 12, 16)                  # decim_rt_radix_ok; 16 is the switch's `default:`
PAIRS = {(500, 100), (125, 80)}                              # fft_kernel.h, RCFM_FFT_DECIM_PAIRS
# fft_kernel.h, RCFM_FFT_FAST_LENGTHS = RCFM_FFT_PAIR_LENGTHS: k_fft_tile2<MidHilbertMask> and k_fft_tile2_pair
FAST_LENGTHS = (75, 80, 100, 120, 125, 128, 150, 160, 192, 200, 240, 250, 256, 300, 320, 375, 384, 400, 480, 500, 512)

# n1: FFT_B's first pass (the tile's lines); L, L2: the tile's two transforms; radices: of the short one, first stage
# first; form: "instantiated" / "run_time", or None -- a separate resample -- with `why` the first rule that refused
Route = collections.namedtuple("Route", "n1 L L2 radices form why")


def _radices(p):
    return tuple(int(p.radix[s]) for s in range(p.nstages))


def _two_pass(B):
    plan = fft_model.describe(B)
    if plan is None or plan.npass != 2:
        return None
    return int(plan.passes[0].L), int(plan.passes[1].L)


def _tile(B, A, lengths):
    """(L2, radices, form or None, why) of B planned as `lengths` = (n1, L): decim_plan, fused_fft_decim_ifft_applies and
    the two kernels' own conditions."""
    n1, L = lengths
    if A % (2 * n1) or A // n1 < 16:
        return A // n1 if A % n1 == 0 else None, (), None, "A %% (2 n1) = %d, A / n1 = %.4g" % (A % (2 * n1), A / n1)
    L2 = A // n1
    pb, pa = fft_model.describe_plan(B, lengths), fft_model.describe_plan(A, (L2, n1))
    if pb is None or pa is None or pa.npass != 2:
        return L2, (), None, "no plan (%d, %d) of A" % (L2, n1)
    d1, d2 = pb.passes[1], pa.passes[0]
    radices = _radices(d2)
    if int(pa.passes[1].L) != n1 or int(d1.L) != L or int(d2.L) != L2:
        return L2, radices, None, "plan lengths"
    same_lines = (d1.load_along_l and not d2.load_along_l and d1.n_inner == d2.n_inner and d1.n_o1 * d1.n_o2 == 1
                  and d2.n_o1 * d2.n_o2 == 1 and d1.out_k == d2.in_l and d2.in_i == 1 and d2.out_i == 1 and d2.has_twiddle)
    if not same_lines:
        return L2, radices, None, "the two passes do not share their lines"
    if (L, L2) in PAIRS:
        return L2, radices, "instantiated", ""
    if L not in RT_LENGTHS:
        return L2, radices, None, "no kernel for L = %d" % L
    if L2 % 2 or L2 < 16 or L2 >= L:
        return L2, radices, None, "L2 = %d against L = %d" % (L2, L)
    if any(r not in RT_RADICES for r in radices):
        return L2, radices, None, "short radices %s" % (radices,)
    return L2, radices, "run_time", ""


def route(kind, B, A):
    """Route of a demodulator-only call, or None where the FFT engine does not serve (B, A) at all (rocFFT)."""
    if fft_model.describe(B) is None or fft_model.describe(A) is None:
        return None
    lengths = _two_pass(B)
    if lengths is None or A >= B or A % 2:
        n1, L = lengths if lengths else (0, 0)
        return Route(n1, L, None, (), None, "A >= B, odd A or no two-pass plan")
    L2, radices, form, why = _tile(B, A, lengths)
    if form is None:
        swapped = (lengths[1], lengths[0])
        if fft_model.describe_plan(B, swapped) is not None:
            alt = _tile(B, A, swapped)
            if alt[2] is not None:
                lengths, (L2, radices, form, why) = swapped, alt
    n1, L = lengths
    if form is not None and kind == "MFM" and A % 4:
        form, why = None, "MFM needs A % 4 == 0"
    if form is not None and kind == "WBFM" and n1 not in FAST_LENGTHS:
        form, why = None, "no two-transform tile of %d points ahead of it" % n1
    return Route(n1, L, L2, radices, form, why)


def pilot_tiles(B):
    """(mask tile length, pair tile length) of the WBFM pilot chain at B -- fused_pilot_chain_applies: a two-pass plan
    (n1, n2) with both lengths specialised runs k_fft_tile2<MidHilbertMask> at n2 and k_fft_tile2_pair at n1 -- or None."""
    lengths = _two_pass(B)
    if lengths is None or lengths[0] not in FAST_LENGTHS or lengths[1] not in FAST_LENGTHS:
        return None
    if fft_model.describe_plan(B, (lengths[1], lengths[0])) is None:
        return None
    return lengths[1], lengths[0]


def seven_smooth(lo, hi):
    """Every 2^a 3^b 5^c 7^d in (lo, hi], ascending."""
    out, stack = set(), [1]
    while stack:
        v = stack.pop()
        for p in (2, 3, 5, 7):
            w = v * p
            if w <= hi and w not in out:
                out.add(w)
                stack.append(w)
    return sorted(v for v in out if v > lo)


# (kind, B, A): (n1, L, L2, radices of the short plan, form) -- what route() must return (tests/test_decim_cases.py: "the
# planner moved this length: exchange it").  B of an FM / MFM row is the smallest bandwidth that reaches its long length
# in the run-time form; the WBFM rows follow the pilot chain's tiles.
# Every comment: bound() as tests/test_length_cases.py prints it, then [measured: rcfm_demod_run on an MI355X against the
# truth, worst of three stations, two buffers and both tile widths, by default; the same with RCFM_OPT_DECIM_TILE = 0
# ("without the tile": on a refused row the same kernels); WBFM: with RCFM_OPT_PILOT_CHAIN = 0].
CASES = {
    # ---- the run-time form, one row per long length no WBFM row below reaches; n1 % 8 != 0 unless noted
    ("FM", 2500, 450): (25, 100, 18, (6, 3), "run_time"),               # bound 1.00e-04 [measured 7.08e-07; without the tile 6.39e-07]
    ("MFM", 3125, 3000): (25, 125, 120, (12, 10), "run_time"),          # bound 1.00e-04 [measured 4.58e-07; without the tile 4.39e-07]
    ("MFM", 5880, 980): (49, 120, 20, (10, 2), "run_time"),             # bound 1.00e-04 [measured 3.58e-07; without the tile 3.43e-07]
    ("FM", 4096, 1024): (32, 128, 32, (8, 4), "run_time"),              # bound 1.00e-04 [measured 4.09e-07; without the tile 3.91e-07]  n1 % 16 == 0
    ("FM", 11250, 3750): (75, 150, 50, (10, 5), "run_time"),            # bound 1.00e-04 [measured 3.44e-07; without the tile 3.98e-07]
    ("MFM", 12800, 5120): (80, 160, 64, (8, 8), "run_time"),            # bound 1.00e-04 [measured 3.68e-07; without the tile 4.14e-07]  n1 % 16 == 0
    ("FM", 12096, 10080): (63, 192, 160, (16, 10), "run_time"),         # bound 1.00e-04 [measured 4.18e-07; without the tile 4.43e-07]  radix 16: the switch's default arm
    ("FM", 98000, 62720): (245, 400, 256, (16, 16), "run_time"),        # bound 1.00e-04 [measured 4.24e-07; without the tile 7.27e-07]
    ("MFM", 164640, 12348): (343, 480, 36, (6, 6), "run_time"),         # bound 1.00e-04 [measured 3.39e-07; without the tile 3.50e-07]
    # ---- the two instantiated pairs
    ("FM", 12500, 8000): (100, 125, 80, (10, 8), "instantiated"),       # bound 1.00e-04 [measured 6.87e-07; without the tile 6.10e-07]
    ("MFM", 125000, 25000): (250, 500, 100, (10, 10), "instantiated"),  # bound 1.00e-04 [measured 5.00e-07; without the tile 5.14e-07]
    # ---- refused neighbours of 12 500 -> 8000: a separate resample
    ("FM", 12500, 11200): (100, 125, 112, (8, 7, 2), None),             # bound 1.00e-04 [measured 6.86e-07; without the tile 6.86e-07]  L2 = 112 has a factor 7
    ("FM", 12500, 8100): (100, 125, 81, (), None),                      # bound 1.00e-04 [measured 6.19e-07; without the tile 6.19e-07]  odd L2: decim_plan refuses, in either order
    ("FM", 12500, 1200): (100, 125, 12, (), None),                      # bound 1.00e-04 [measured 4.31e-07; without the tile 4.31e-07]  A / n1 < 16
    # ---- WBFM: per length of the pilot chain's two tiles the smallest bandwidth that runs it (pilot_tile_bandwidths)
    ("WBFM", 38400, 19200): (160, 240, 120, (12, 10), "run_time"),      # bound 1.00e-04 [measured 1.71e-06; without the tile 1.71e-06; without the pilot chain 1.81e-06]
    ("WBFM", 40000, 8000): (160, 250, 50, (10, 5), "run_time"),         # bound 1.00e-04 [measured 2.31e-06; without the tile 2.22e-06; without the pilot chain 2.17e-06]
    ("WBFM", 40960, 30720): (160, 256, 192, (16, 12), "run_time"),      # bound 4.65e-05 [measured 1.47e-06; without the tile 1.53e-06; without the pilot chain 1.56e-06]
    ("WBFM", 45000, 10800): (120, 375, 90, (10, 3, 3), "run_time"),     # bound 1.00e-04 [measured 8.51e-07; without the tile 8.51e-07; without the pilot chain 5.90e-07]  n1 % 16 == 8; the four-stage long length
    ("WBFM", 46080, 18432): (192, 240, 96, (8, 6, 2), "run_time"),      # bound 1.00e-04 [measured 9.00e-07; without the tile 8.25e-07; without the pilot chain 6.64e-07]
    ("WBFM", 48000, 12960): (240, 200, 54, (6, 3, 3), "run_time"),      # bound 1.00e-04 [measured 8.20e-07; without the tile 8.20e-07; without the pilot chain 7.80e-07]  alloc()'s swap: planned 200 x 240, run as 240 x 200
    ("WBFM", 72000, 24000): (240, 300, 100, (10, 10), "run_time"),      # bound 1.00e-04 [measured 7.71e-07; without the tile 7.71e-07; without the pilot chain 4.11e-07]
    ("WBFM", 73728, 24576): (192, 384, 128, (8, 8, 2), "run_time"),     # bound 1.00e-04 [measured 8.69e-07; without the tile 8.69e-07; without the pilot chain 4.95e-07]
    ("WBFM", 76800, 19200): (240, 320, 80, (10, 8), "run_time"),        # bound 1.00e-04 [measured 6.80e-07; without the tile 6.60e-07; without the pilot chain 4.81e-07]
    ("WBFM", 100000, 16000): (400, 250, 40, (10, 4), "run_time"),       # bound 1.00e-04 [measured 9.92e-07; without the tile 9.92e-07; without the pilot chain 7.78e-07]
    ("WBFM", 125000, 15000): (250, 500, 60, (10, 6), "run_time"),       # bound 1.00e-04 [measured 3.86e-07; without the tile 5.24e-07; without the pilot chain 5.24e-07]
    ("WBFM", 131072, 18432): (256, 512, 72, (8, 3, 3), "run_time"),     # bound 1.00e-04 [measured 5.46e-07; without the tile 5.26e-07; without the pilot chain 5.07e-07]
    ("WBFM", 180000, 23040): (480, 375, 48, (8, 6), "run_time"),        # bound 1.00e-04 [measured 6.02e-07; without the tile 6.54e-07; without the pilot chain 1.05e-06]
    # ---- WBFM at B % 4 != 0 (the generic pilot kernels): the only bandwidths whose plans hold 125 and 150 points
    ("WBFM", 46875, 20000): (125, 375, 160, (16, 10), "run_time"),      # bound 1.00e-04 [measured 5.17e-07; without the tile 5.14e-07; without the pilot chain 5.78e-07]
    ("WBFM", 56250, 16200): (150, 375, 108, (6, 6, 3), "run_time"),     # bound 1.00e-04 [measured 7.22e-06; without the tile 7.34e-06; without the pilot chain 5.17e-06]
}
WBFM_MIN_B, MAX_B = 38100, 262144       # the pilot band-pass needs 19 050 Hz below B / 2; no test here goes beyond 2^18


def tile_of(kind, B, A):
    """(form, L, L2) of a row that takes the tile, else None (length_cases.tile_of's counterpart for this table)."""
    n1, L, L2, _, form = CASES[(kind, B, A)]
    return (form, L, L2) if form else None


def pilot_tiles_of(kind, B, A):
    """(mask tile length, pair tile length) the pilot chain of a WBFM row runs -- in the order of B's two lengths that the
    route takes (alloc()'s swap exchanges the two roles) --, or None."""
    r = route(kind, B, A)
    if kind != "WBFM" or r is None or r.n1 not in FAST_LENGTHS or r.L not in FAST_LENGTHS:
        return None
    if fft_model.describe_plan(B, (r.L, r.n1)) is None:
        return None
    return r.L, r.n1


def pilot_tile_bandwidths():
    """{tile length: smallest 7-smooth B in (WBFM_MIN_B, MAX_B] with B % 4 == 0 whose two-pass plan has both lengths
    specialised and this one among them} -- from rcfm_fft_describe alone."""
    first = {}
    for B in seven_smooth(WBFM_MIN_B, MAX_B):
        tiles = pilot_tiles(B) if B % 4 == 0 else None
        for L in tiles or ():
            first.setdefault(L, B)
    return first


def reachable():
    """What demodulator geometries can reach, from rcfm_fft_describe alone: {"mask": lengths of k_fft_tile2<MidHilbertMask>,
    "pair": of k_fft_tile2_pair, "run_time": long lengths of k_fft_tile2_decim_rt, "instantiated": (L, L2) pairs}, over
    every 7-smooth B from 2000 (WBFM: above WBFM_MIN_B; B % 4 is no condition of fused_pilot_chain_applies) to MAX_B.
    Both orders of B's two lengths count, whether or not some A makes alloc() take the other one: what is missing here
    cannot run, what is listed runs in a row of CASES or of the older geometry tests."""
    out = {"mask": set(), "pair": set(), "run_time": set(), "instantiated": set()}
    for B in seven_smooth(1999, MAX_B):
        lengths = _two_pass(B)
        if lengths is None:
            continue
        if B > WBFM_MIN_B:
            for n1, n2 in (lengths, lengths[::-1]):          # the swap exchanges the roles
                if n1 in FAST_LENGTHS and n2 in FAST_LENGTHS and fft_model.describe_plan(B, (n2, n1)) is not None \
                        and fft_model.describe_plan(B, (n1, n2)) is not None:
                    out["mask"].add(n2)
                    out["pair"].add(n1)
        for n1, L in (lengths, lengths[::-1]):
            if L in RT_LENGTHS and fft_model.describe_plan(B, (n1, L)) is not None:
                # one L2 per radix list is enough to know that the length is reached: the smallest, 16 = 8 x 2
                if _tile(B, 16 * n1, (n1, L))[2] == "run_time":
                    out["run_time"].add(L)
            for pl, pl2 in PAIRS:
                if L == pl and _tile(B, pl2 * n1, (n1, L))[2] == "instantiated":
                    out["instantiated"].add((pl, pl2))
    return out


MUTANT = "n/2 not doubled"      # length_cases.mutants: the one rule the decimating tile restates (its Nyquist merge)


def bound(kind, B, A):
    """min(TOL, closest "n/2 not doubled" mutant / 10) over the case's stations and buffers (length_cases.bound)."""
    return lc.bound(kind, B, A, MUTANT)
