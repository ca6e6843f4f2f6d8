"""The option of the packed observation passes' load order ("packed_prefetch") is handled by ps_set_option ahead of the option
table, as "rows_regs" and "cg_persist_recover" are (tests/test_options_host.py pins the table's rows to the chain it replaced).
No GPU: the sources, the public header and the binding are read and held together -- the name is set, read back and documented,
it is not also a row of the table, every packed launch chooses its instantiation by it, and the parity tap the GPU test uses is
declared where the binding expects it."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'packed_prefetch'


def read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def test_the_name_is_set_read_back_and_documented():
    solver = read('pyslam_amd', 'csrc', 'ps_abi_solver.h')
    setter = re.search(r'int ps_set_option\(.*?\n}\n', solver, re.S).group(0)
    getter = re.search(r'int ps_get_option\(.*?\n}\n', solver, re.S).group(0)
    assert 0 < setter.index('"%s"' % NAME) < setter.index('ps_option_apply(')          # ahead of the table
    assert 'n == "%s"' % NAME in getter
    header = read('include', 'pyslam_hip.h')
    assert '"%s"' % NAME in re.search(r'/\* Tuning knobs.*?\*/\s*int ps_set_option', header, re.S).group(0)
    assert '"%s"' % NAME in re.search(r'int ps_set_option.*?int ps_get_option', header, re.S).group(0)
    assert '"%s"' % NAME not in read('pyslam_amd', 'csrc', 'ps_options.h')
    assert 'int packed_prefetch = 1;' in read('pyslam_amd', 'csrc', 'ps_core.hip')      # default on


def test_every_packed_launch_chooses_by_the_option():
    """Four launch sites (landmark pass, landmark pass with the cost, cost pass, back-substitution): each names both forms."""
    host = read('pyslam_amd', 'csrc', 'ps_host_cg.h')
    for macro in ('PS_LMP_LAUNCH', 'PS_LMC_LAUNCH', 'PS_CSP_LAUNCH'):
        uses = re.findall(r'%s\((?:true|false), (true|false)\)' % macro, host)
        assert sorted(uses) == ['false', 'false', 'true', 'true'], macro
    assert 'if (h->packed_prefetch) PS_BSP_LAUNCH1(MD, true, __VA_ARGS__); else PS_BSP_LAUNCH1(MD, false, __VA_ARGS__);' in host
    assert len(re.findall(r'h->packed_prefetch', host)) == 4


def test_the_parity_tap_is_declared_and_bound():
    from pyslam_amd import _native
    header = read('include', 'pyslam_hip.h')
    decl = re.search(r'int ps_debug_packed_runs\((.*?)\);', header, re.S).group(1)
    assert len(decl.split(',')) == len(_native.SIGNATURES['ps_debug_packed_runs'][1]) == 7
    assert 'int ps_debug_packed_runs(' in read('pyslam_amd', 'csrc', 'ps_abi_solver.h')
