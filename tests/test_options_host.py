"""The option table (pyslam_amd/csrc/ps_options.h, compiled here with a plain C++ compiler: no HIP, no GPU) against a literal
transcription of the if / else-if chain that ps_set_option was before the table: every name, its default, how a value is stored
(truncated, or != 0), the first value refused on either side with the chain's own words, and what the change invalidates.  The
table below is written out by hand on purpose: it is not read from the header."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
COARSE, FACTOR, SIDE, RELOOK, LDI_OFF = 1, 2, 4, 8, 16          # coarse_built = false | lci_next = -1 | side_todo = false | relook_path | drop the inverse when switched off
UNKNOWN, REFUSED = -1, -2
ABLATION = ': timing experiments exist in the measurement build only (__graft_entry__.build_measure(), PYSLAM_AMD_MEASURE=1)'

# name: (default, kind, lowest accepted, highest accepted, refusal, effects)
#   bool   stored as value != 0                       int    stored truncated, nothing refused
#   range  refused below lo / above hi, else truncated    below  as range, but hi itself is the first refused value
#   exact  only the integers lo .. hi                 uint   range, into an unsigned
#   tol    a double, refused unless >= 0 (NaN too)    tri    ldi_direct: ok = value != 0, on = value > 0
#   ablation  product build: 0 is a no-op, anything else refused; measurement build: int
CHAIN = {
    'pcg_variant': (1, 'exact', 0, 1, 'pcg_variant must be 0 or 1', 0),
    'coarse_groups': (-1, 'below', -1, 1024, 'coarse_groups out of range (-1 auto, 0 off, else number of hat intervals; above 63 only '
                      'for the explicit two-level PCG, at most 1023)', COARSE),
    'cg_ablate': (0, 'ablation', None, None, 'cg_ablate' + ABLATION, 0),
    'schur_ablate': (0, 'ablation', None, None, 'schur_ablate' + ABLATION, 0),
    'lm_ablate': (0, 'ablation', None, None, 'lm_ablate' + ABLATION, 0),
    'schur_pipeline': (1, 'bool', None, None, None, 0),
    'coarse_lag': (1, 'bool', None, None, None, 0),
    'cg_force_restart': (0, 'bool', None, None, None, 0),
    'cg_force_breakdown': (0, 'int', None, None, None, 0),
    'xcg_restrict_fused': (1, 'bool', None, None, None, 0),
    'band_chol': (1, 'bool', None, None, None, FACTOR),
    'lm_packed': (1, 'bool', None, None, None, 0),
    'pose_xcd': (1, 'bool', None, None, None, 0),
    'fuse_cost': (1, 'int', None, None, None, 0),
    'sync_refactor': (1, 'bool', None, None, None, 0),
    'hold_across_steps': (1, 'bool', None, None, None, 0),
    'band_part': (1, 'bool', None, None, None, FACTOR),
    'band_part_chunk': (0, 'range', 0, 4096, 'band_part_chunk must be 0 (automatic) .. 4096 nodes', FACTOR),
    'coarse_auto_hold': (1, 'bool', None, None, None, 0),
    'coarse_adaptive_hold': (1, 'bool', None, None, None, 0),
    'xcg_fused': (1, 'exact', 0, 2, 'xcg_fused must be 0, 1 or 2', 0),
    'lagged_inverse': (1, 'bool', None, None, None, LDI_OFF | RELOOK),
    'ldi_max_unknowns': (2048, 'range', 0, 3328, 'ldi_max_unknowns out of range (0 .. 3328)', RELOOK),
    'ldi_cap': (12, 'range', 1, 64, 'ldi_cap out of range (1 .. 64)', 0),
    'ldi_cost_tol': (0.05, 'tol', 0, INF, 'ldi_cost_tol must be >= 0', 0),
    'ldi_refresh_its': (7, 'range', 0, 64, 'ldi_refresh_its out of range (0 .. 64)', 0),
    'ldi_direct': (-1, 'tri', None, None, None, 0),
    'direct_fused': (1, 'bool', None, None, None, 0),
    'ldi_seed_lag': (1, 'range', 1, 16, 'ldi_seed_lag out of range (1 .. 16)', 0),
    'ldi_seed_steps': (3, 'range', 1, 40, 'ldi_seed_steps out of range (1 .. 40)', 0),
    'coarse_refresh_every': (1, 'range', 1, 16, 'coarse_refresh_every must be 1..16', 0),
    'coarse_lag_x': (1, 'bool', None, None, None, FACTOR | SIDE),
    'cg_lds': (1, 'bool', None, None, None, 0),
    'cg_persist': (1, 'bool', None, None, None, 0),
    'xcg_persist': (1, 'bool', None, None, None, 0),
    'cg_persist_spin': (200000, 'uint', 0, 1e7, 'cg_persist_spin out of range', 0),
    'cg_explicit': (1, 'bool', None, None, None, COARSE),
    'big_chol': (1, 'bool', None, None, None, 0),
    'fused_motion_only': (1, 'bool', None, None, None, 0),
    'direct_max_unknowns': (90, 'range', 0, 90, 'direct_max_unknowns must be 0..90', 0),
    'coarse_basis': (1, 'bool', None, None, None, FACTOR | SIDE),
    'profile_every': (1, 'range', 1, INF, 'profile_every must be >= 1', 0),
    'cg_margin': (4, 'range', 0, 64, 'cg_margin out of range', 0),
    'cg_split_min_rows': (1024, 'int', None, None, None, COARSE),
    'cg_explicit_min_rows': (-1, 'int', None, None, None, COARSE),
    'pcg_chunk': (8, 'range', 1, 4096, 'pcg_chunk out of range', 0),
    'lin_zero_list': (1, 'bool', None, None, None, 0),
}
# tested by ps_set_option ahead of the table (a caller's loop sets both per iteration: nothing is invalidated, nothing looked up)
EARLY = ('expect_next', 'solve_horizon')
REMOVED = ('schur_mode', 'schur_stream', 'xcg_persist4', 'cg_pipelined', 'pose_async')      # tests/test_gpu_edges.py


class Table:
    def __init__(self, so):
        self.so = so
        so.opt_name.restype = C.c_char_p
        so.opt_get.restype = C.c_double
        so.opt_get.argtypes = [C.c_void_p, C.c_char_p]
        so.opt_apply.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.POINTER(C.c_char_p)]
        so.opt_fresh.argtypes = [C.c_void_p]
        so.opt_ldi_possible.argtypes = [C.c_void_p, C.c_long]
        self.names = [so.opt_name(i).decode() for i in range(so.opt_count())]

    def fresh(self):
        buf = C.create_string_buffer(self.so.opt_size())
        self.so.opt_fresh(buf)
        return buf

    def apply(self, buf, name, value):
        """-> (effects mask | UNKNOWN | REFUSED, refusal text or None)"""
        msg = C.c_char_p()
        rc = self.so.opt_apply(buf, name.encode(), value, C.byref(msg))
        return rc, (msg.value.decode() if rc == REFUSED else None)

    def get(self, buf, name):
        return self.so.opt_get(buf, name.encode())


@pytest.fixture(scope='module', params=['product', 'measure'])
def table(request, tmp_path_factory):
    """The header in a shared library, once as the product build and once with -DPS_MEASURE (the project needs a C++ compiler to
    build at all: a missing one is a failure)."""
    lib = str(tmp_path_factory.mktemp('options') / 'shim.so')
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-O1', '-shared', '-fPIC'] +
                   (['-DPS_MEASURE'] if request.param == 'measure' else []) +
                   ['-I' + os.path.join(REPO, 'pyslam_amd', 'csrc'), os.path.join(REPO, 'tests', 'options_shim.cpp'), '-o', lib], check=True)
    t = Table(C.CDLL(lib))
    t.measure = request.param == 'measure'
    assert t.so.opt_codes() == (-UNKNOWN) | (-REFUSED) << 4
    assert t.so.opt_effect_bits() == COARSE | FACTOR << 4 | SIDE << 8 | RELOOK << 12 | LDI_OFF << 16
    return t


def test_the_names_are_the_chains(table):
    assert len(table.names) == len(set(table.names))               # no name twice
    assert set(table.names) == set(CHAIN)
    # 46 in the table + the two early names = the 48 names the chain compared against (in both builds); + the test hook
    # "cg_force_breakdown", which the chain never had
    assert len(CHAIN) == 47 and not set(EARLY) & set(CHAIN)
    for name in REMOVED + EARLY + ('', 'pcg_variant ', 'PCG_VARIANT'):
        buf = table.fresh()
        before = buf.raw
        assert table.apply(buf, name, 0.) == (UNKNOWN, None) and buf.raw == before


def test_every_name_is_documented_in_the_public_header(table):
    with open(os.path.join(REPO, 'include', 'pyslam_hip.h')) as f:
        comment = re.search(r'/\* Tuning knobs.*?\*/\s*int ps_set_option', f.read(), re.S).group(0)
    for name in table.names + list(EARLY):
        assert '"%s"' % name in comment, name


def accepted_and_refused(kind, lo, hi):
    """[(value, what the chain stored)], [refused values] for one row."""
    nxt = math.nextafter
    if kind == 'bool':
        return [(0., 0), (1., 1), (-2.5, 1), (0.25, 1), (-0., 0), (math.nan, 1)], []
    if kind == 'int':
        return [(0., 0), (3.9, 3), (-2.7, -2), (-1., -1), (100000., 100000)], []
    if kind == 'tri':
        return [(-1., -1), (0., 0), (1., 1), (0.5, 1), (-3., -1), (-0., 0)], []
    if kind == 'tol':
        return [(0., 0.), (0.05, 0.05), (1e300, 1e300), (-0., 0.), (INF, INF)], [-1e-300, -1., math.nan, -INF]
    if kind == 'exact':
        return [(float(v), v) for v in range(lo, hi + 1)], [lo - 1., hi + 1., lo + 0.5, nxt(float(hi), INF), math.nan]
    if kind == 'below':
        return [(float(lo), lo), (hi - 1., hi - 1), (hi - 0.5, hi - 1), (-0.5, 0), (5.9, 5)], [lo - 1., nxt(float(lo), -INF), float(hi), hi + 1.]
    assert kind in ('range', 'uint')
    ok = [(float(lo), int(lo)), (lo + 0.75, int(lo))]
    bad = [lo - 1., nxt(float(lo), -INF)]
    if hi == INF:
        ok += [(1e6, 1000000)]
    else:
        ok += [(float(hi), int(hi)), (hi - 0.5, int(hi) - 1)]
        bad += [hi + 1., nxt(float(hi), INF)]
    return ok, bad


@pytest.mark.parametrize('name', sorted(CHAIN))
def test_a_row_against_the_chain(table, name):
    default, kind, lo, hi, refusal, effects = CHAIN[name]
    if kind == 'ablation':
        kind = 'int' if table.measure else 'noop'
    assert table.get(table.fresh(), name) == default
    if kind == 'noop':                                              # product build: 0 changes nothing, anything else is refused
        buf = table.fresh()
        before = buf.raw
        assert table.apply(buf, name, 0.) == (0, None) and buf.raw == before
        for v in (1., -1., 0.5, math.nan):
            assert table.apply(buf, name, v) == (REFUSED, refusal) and buf.raw == before
        return
    ok, bad = accepted_and_refused(kind, lo, hi)
    for value, stored in ok:
        buf = table.fresh()
        assert table.apply(buf, name, value) == (effects, None), value
        assert table.get(buf, name) == stored, value
    for value in bad:
        buf = table.fresh()
        assert table.apply(buf, 'pcg_chunk' if name == 'cg_margin' else 'cg_margin', 9.) == (0, None)     # (a struct that is not all defaults)
        before = buf.raw
        assert table.apply(buf, name, value) == (REFUSED, refusal), value
        assert buf.raw == before, value


def test_a_row_writes_its_own_member_only(table):
    """Every name set to a non-default value on one struct, in table order: each reads back its own value at the end, so no
    two names share a member."""
    other = {'bool': lambda d: 1 - d, 'int': lambda d: d + 7, 'range': lambda d: d + 1 if d < 16 else d - 1, 'below': lambda d: 33,
             'exact': lambda d: 0, 'uint': lambda d: 1234, 'tol': lambda d: 0.25, 'tri': lambda d: 0}
    buf, want = table.fresh(), {}
    for name in table.names:
        default, kind = CHAIN[name][:2]
        if kind == 'ablation':
            if not table.measure:
                continue
            kind = 'int'
        want[name] = other[kind](default)
        assert want[name] != default
        assert table.apply(buf, name, float(want[name]))[0] >= 0
    for name, v in want.items():
        assert table.get(buf, name) == v, name


def test_where_the_lagged_inverse_can_apply(table):
    """n <= ldi_max_unknowns, n <= 3328, n > direct_max_unknowns, and the option on: the one expression behind build_coarse's
    crossover, relook_path and ldi_eligible."""
    buf = table.fresh()
    assert [table.so.opt_ldi_possible(buf, n) for n in (90, 91, 2048, 2049)] == [0, 1, 1, 0]
    table.apply(buf, 'ldi_max_unknowns', 3328.)
    table.apply(buf, 'direct_max_unknowns', 0.)
    assert [table.so.opt_ldi_possible(buf, n) for n in (0, 1, 3328, 3329)] == [0, 1, 1, 0]
    table.apply(buf, 'lagged_inverse', 0.)
    assert not table.so.opt_ldi_possible(buf, 1000)
