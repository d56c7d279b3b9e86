"""CPU: tests/decim_cases.py -- the decimating tile's routing restated, its table and what the table covers.

    constants     the kernel lists decim_cases restates are the ones the headers instantiate (read from csrc/*.h)
    routing       route() gives the routes the suite already documents, and every row of the table is what route() says
                  ("the planner moved this length: exchange it")
    coverage      every long length of the run-time kernel, both instantiated pairs, every run-time radix, the three
                  classes of n1 (ragged last tile at either width), two-, three- and four-stage long lengths, MFM and WBFM
                  rows, alloc()'s swap, the three refused neighbours; per length of the WBFM pilot chain's tiles the
                  smallest bandwidth that runs it.  Each row is the only one that provides something: no row can go
    unreachable   which instantiated lengths no demodulator geometry reaches (DESIGN.md section 3.2 lists them)
The conditioning of every row (reference within bound / 10, phase steps, clipping) is tests/test_length_cases.py's
per-case test, which runs over this table too.
"""

import os
import re

import decim_cases as dc
import length_cases as lc
from conftest import ROOT

CSRC = os.path.join(ROOT, "radio-core_amd", "csrc")


def _macro(header, name):
    """The X(...) rows of `#define name(X) ...` in csrc/header, as tuples of ints (continuation lines joined)."""
    text = open(os.path.join(CSRC, header)).read().replace("\\\n", " ")
    body = re.search(r"^#define %s\(X(?:, LONGT)?\)(.*)$" % name, text, re.M)
    assert body, (header, name)
    return [tuple(int(v) for v in row.split(",")) for row in re.findall(r"X\(([0-9, ]+)\)", body.group(1))]


def test_restated_kernel_lists_are_the_headers():
    rt = _macro("fft_decim_rt.h", "RCFM_FFT_DECIM_RT_LENGTHS")
    assert {r[0]: tuple(v for v in r[1:] if v > 1) for r in rt} == dc.RT_LENGTHS and len(rt) == 19
    text = open(os.path.join(CSRC, "fft_decim_rt.h")).read()
    ok = re.search(r"decim_rt_radix_ok\(int r\) \{\s*return ([^;]+);", text).group(1)
    assert tuple(int(v) for v in re.findall(r"r == (\d+)", ok)) == dc.RT_RADICES
    cases = [int(v) for v in re.findall(r"case (\d+): stage_rt<\1, T>", text)]
    assert cases == [r for r in dc.RT_RADICES if r != 16] and "default: stage_rt<16, T>" in text
    # the two-transform tiles: 18 lengths, the long table (480, 500) and 512
    fast = [r[0] for r in _macro("fft_kernel.h", "RCFM_FFT_LENGTHS_")] + [r[0] for r in _macro("fft_kernel.h", "RCFM_FFT_LONG_TABLE")]
    assert sorted(fast) == list(dc.FAST_LENGTHS) and len(fast) == 21
    kernel = open(os.path.join(CSRC, "fft_kernel.h")).read()
    assert "RCFM_FFT_DECIM_X_(X, 500, 25, 20, 1, 1, 100, RCFM_DECIM_100)" in kernel and "X(125, 5, 5, 5, 1, 80, 10, 8, 1)" in kernel
    assert dc.PAIRS == {(500, 100), (125, 80)}


def test_routes_the_suite_documents():
    """tests/test_hip_configs.py, test_hip_lengths.py, test_hip_am.py: 240 000 -> 48 000 instantiated, 60 000 -> 12 000 as
    250 -> 50, 256 000 -> 32 000 as 512 -> 64 after the swap, 23 625 -> 8000 with no tile, 25 000 -> 8000 with it."""
    assert dc.route("WBFM", 240000, 48000)[:5] == (480, 500, 100, (10, 10), "instantiated")
    assert dc.route("WBFM", 60000, 12000)[:5] == (240, 250, 50, (10, 5), "run_time")
    assert dc.route("WBFM", 256000, 32000)[:5] == (500, 512, 64, (8, 8), "run_time")
    assert dc._two_pass(256000) == (512, 500)                                       # ... which the planner orders the other way
    assert dc.route("FM", 23625, 8000).form is None and dc.route("FM", 23625, 8000).L == 189
    assert dc.route("AM", 25000, 8000).form == "run_time"
    assert dc.route("FM", 24001, 8000) is None                                      # rocFFT
    assert dc.route("MFM", 2500, 450).form is None and dc.route("FM", 2500, 450).form == "run_time"   # MFM: A % 4 == 0


def test_table_is_what_the_routing_says():
    for (kind, B, A), row in dc.CASES.items():
        r = dc.route(kind, B, A)
        assert r is not None, (kind, B, A, "the engine plans neither length: exchange it")
        assert tuple(r[:5]) == row, (kind, B, A, r, "the planner moved this length: exchange it")
        assert B <= dc.MAX_B and lc.branch(B, A) == "down_even"
        assert dc.tile_of(kind, B, A) == ((row[4], row[1], row[2]) if row[4] else None)
        if kind == "WBFM":
            assert B > dc.WBFM_MIN_B


def _rows(form=None, kind=None):
    return {c: v for c, v in dc.CASES.items() if (form is None or v[4] == form) and (kind is None or c[0] == kind)}


def _only_row(rows, what):
    assert len(rows) == 1, (what, sorted(rows))
    return next(iter(rows))


def test_table_covers_the_kernels():
    rt = _rows("run_time")
    # every long length of the run-time kernel, with the radix list its instantiation has
    assert {v[1] for v in rt.values()} == set(dc.RT_LENGTHS), sorted(set(dc.RT_LENGTHS) - {v[1] for v in rt.values()})
    assert {len(dc.RT_LENGTHS[v[1]]) for v in rt.values()} == {2, 3, 4}
    assert any(v[1] == 375 for v in rt.values())                                    # the four-stage one
    # both instantiated pairs; 12 500 -> 8000 is 125 -> 80
    assert {(v[1], v[2]) for v in _rows("instantiated").values()} == dc.PAIRS
    assert dc.CASES[("FM", 12500, 8000)][1:3] == (125, 80)
    # every run-time radix in some short plan: 12 and 16 from specialised lists, 3 from lengths such as 18, 54 and 90
    seen = {r for v in rt.values() for r in v[3]}
    assert seen == set(dc.RT_RADICES), sorted(set(dc.RT_RADICES) - seen)
    assert all(set(v[3]) <= set(dc.RT_RADICES) and v[2] % 2 == 0 and 16 <= v[2] < v[1] for v in rt.values())
    assert {len(v[3]) for v in rt.values()} >= {2, 3}                               # two and three run-time stages
    # the lines: whole tiles at both widths, a ragged last tile at 16 lines only, at both
    for want in (lambda n1: n1 % 16 == 0, lambda n1: n1 % 16 == 8, lambda n1: n1 % 8 != 0):
        assert any(want(v[0]) for v in rt.values())
    # kinds: MFM rides on pairs like FM but needs A % 4 == 0; WBFM runs one complex signal per channel
    mfm, wbfm = _rows(kind="MFM"), _rows(kind="WBFM")
    assert len(mfm) >= 4 and all(A % 4 == 0 for _, _, A in mfm) and sum(v[4] == "run_time" for v in mfm.values()) >= 2
    assert len(wbfm) >= 4 and all(v[4] == "run_time" for v in wbfm.values())
    # alloc()'s swap: one row runs B in the other order than the planner's
    assert any(dc._two_pass(B) == (v[1], v[0]) and v[1] != v[0] for (_, B, _), v in rt.items())


def test_refused_neighbours_are_in_the_table():
    import fft_model
    refused = {c: v for c, v in dc.CASES.items() if v[4] is None}
    whys = {c: dc.route(*c).why for c in refused}
    seven = {c for c, v in refused.items() if any(r == 7 for r in v[3])}
    odd = {c for c, v in refused.items() if v[2] % 2 == 1}
    short = {c for c, v in refused.items() if v[2] < 16}
    assert len(seven) == 1 and len(odd) == 1 and len(short) == 1 and len(refused) == 3, whys
    assert ("FM", 12500, 11200) in seven
    for kind, B, A in refused:          # neighbours of 12 500 -> 8000 that stay on the engine: a separate resample, no rocFFT
        assert (kind, B) == ("FM", 12500) and fft_model.describe(A) is not None and A % 2 == 0 and A < B


def test_no_row_can_go():
    """Each row is the only one that provides something the tests above ask for."""
    rt = _rows("run_time")
    needed = set()
    for L in dc.RT_LENGTHS:                                     # FM / MFM rows: the only row of their long length
        rows = {c for c, v in rt.items() if v[1] == L}
        if len(rows) == 1:
            needed |= rows
    needed |= set(_rows("instantiated")) | {c for c, v in dc.CASES.items() if v[4] is None}
    first = dc.pilot_tile_bandwidths()                          # WBFM rows: the smallest bandwidth of some tile length ...
    needed |= {c for c in _rows(kind="WBFM") if c[1] in first.values()}
    reach = dc.reachable()
    for L in (reach["mask"] | reach["pair"]) - set(first):      # ... or the only row with a length B % 4 == 0 never has
        needed.add(_only_row({c for c in _rows(kind="WBFM") if L in (dc.pilot_tiles_of(*c) or ())}, L))
    assert needed == set(dc.CASES), sorted(set(dc.CASES) - needed)


def test_wbfm_rows_reach_every_pilot_tile_length():
    """Per length of k_fft_tile2<MidHilbertMask> / k_fft_tile2_pair that a 7-smooth WBFM bandwidth with B % 4 == 0 reaches, the
    table has the smallest such bandwidth, with an A that takes the decimating tile behind the pilot chain; the lengths
    that only B % 4 != 0 reaches (the generic pilot kernels) have a row too."""
    first = dc.pilot_tile_bandwidths()
    assert sorted(first) == [120, 160, 192, 200, 240, 250, 256, 300, 320, 375, 384, 400, 480, 500, 512], sorted(first)
    rows = _rows(kind="WBFM")
    have = {}
    for (kind, B, A) in rows:
        tiles = dc.pilot_tiles_of(kind, B, A)
        assert tiles is not None and set(tiles) == set(dc.pilot_tiles(B)), (B, A, tiles)
        for L in tiles:
            have.setdefault(L, set()).add(B)
    for L, B in first.items():
        assert B in have.get(L, ()), (L, B, "the planner moved this length: exchange it")
    reach = dc.reachable()
    assert set(have) == reach["mask"] | reach["pair"], (sorted(have), reach)
    # the padded audio rows of fused_fft_decim_ifft (demod.hip, audio_pitch: even n1, no multiple of 16) and the plain ones
    assert any(v[0] % 16 and v[0] % 2 == 0 for v in rows.values()) and any(v[0] % 16 == 0 for v in rows.values())


def test_blocked_layout_of_the_wbfm_rows():
    """length_cases.blocked_layout on the order of B's lengths that the route runs: the GPU test holds the effective
    RCFM_OPT_PILOT_BLOCKED to it.  Both answers occur."""
    import fft_model
    seen = set()
    for (kind, B, A), v in _rows(kind="WBFM").items():
        seen.add(bool(B % 4 == 0 and lc.blocked_layout(fft_model.describe_plan(B, (v[0], v[1])))))
    assert seen == {True, False}


def test_lengths_no_demodulator_geometry_reaches():
    """From rcfm_fft_describe alone (decim_cases.reachable: every 7-smooth bandwidth up to 262 144, either order of its two
    pass lengths).  DESIGN.md section 3.2 lists these; the instantiations stay."""
    reach = dc.reachable()
    fast = set(dc.FAST_LENGTHS)
    assert sorted(fast - reach["mask"]) == [75, 80, 100, 128]
    assert sorted(fast - reach["pair"]) == [75, 80, 100, 128]
    assert sorted(set(dc.RT_LENGTHS) - reach["run_time"]) == []
    assert reach["instantiated"] == dc.PAIRS
    # 125 and 150 points: only at bandwidths with B % 4 != 0
    first = dc.pilot_tile_bandwidths()
    assert sorted((reach["mask"] | reach["pair"]) - set(first)) == [125, 150]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "no demodulator geometry reaches 75, 80, 100 or 128 points" in design
