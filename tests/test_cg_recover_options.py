"""The options of the one-launch folded CG's recovery ("cg_persist_recover", "cg_persist_recover_lds") are handled by
ps_set_option ahead of the option table, as "setup_ride" and "rows_regs" are (tests/test_options_host.py pins the table's rows to the
if / else-if chain it replaced, so a name that came later is not a row).  No GPU: the sources and the public header are read and
held together -- every name set or read back is documented, the cap the header states is the one the kernel's header derives, and
neither name is also a row of the table."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET = ('cg_persist_recover', 'cg_persist_recover_lds')
READ = SET + ('cg_persist_recover_need', 'cg_persist_recovered', 'cg_persist_recover_fallbacks')


def read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def test_the_names_are_set_read_back_and_documented():
    solver = read('pyslam_amd', 'csrc', 'ps_abi_solver.h')
    setter = re.search(r'int ps_set_option\(.*?\n}\n', solver, re.S).group(0)
    getter = re.search(r'int ps_get_option\(.*?\n}\n', solver, re.S).group(0)
    table_call = setter.index('ps_option_apply(')
    for name in SET:
        assert 0 < setter.index('"%s"' % name) < table_call, name       # ahead of the table
    for name in READ:
        assert 'n == "%s"' % name in getter, name
    header = read('include', 'pyslam_hip.h')
    knobs = re.search(r'/\* Tuning knobs.*?\*/\s*int ps_set_option', header, re.S).group(0)
    readback = re.search(r'int ps_set_option.*?int ps_get_option', header, re.S).group(0)
    for name in SET:
        assert '"%s"' % name in knobs, name
    for name in READ:
        assert '"%s"' % name in readback, name
    table = read('pyslam_amd', 'csrc', 'ps_options.h')
    for name in READ:
        assert '"%s"' % name not in table, name


def test_the_documented_cap_is_the_derived_one():
    kernel = read('pyslam_amd', 'csrc', 'ps_k_cg_persist.h')
    m = re.search(r'#define PS_CP_RECOVER_LDS_CAP \(\((\d+) - (\d+)\) \* 1024\)', kernel)
    cap = (int(m.group(1)) - int(m.group(2))) * 1024
    assert int(m.group(1)) == 160                                        # LDS of a gfx950 compute unit, KB
    # the static LDS the kernel keeps: rn (PS_CP_NV * PS_CP_NT + 2 doubles) and red (2 x 2 x 8 doubles), rounded up to whole KB
    static = (4 * 512 + 2) * 8 + 2 * 2 * 8 * 8
    assert static % 16 == 0 and -(-static // 1024) == int(m.group(2))
    header = read('include', 'pyslam_hip.h')
    assert '"cg_persist_recover_lds" [%d; 0 .. %d bytes' % (cap, cap) in header
    assert 'cg_persist_recover_lds out of range (0 .. %d bytes)' % cap in read('pyslam_amd', 'csrc', 'ps_abi_solver.h')
    assert 'int cg_persist_recover_lds = PS_CP_RECOVER_LDS_CAP;' in read('pyslam_amd', 'csrc', 'ps_core.hip')
