"""The option of the pose pass's load order and accumulation ("pose_prefetch") is handled by ps_set_option ahead of the option
table, as "rows_regs" and "packed_prefetch" are (tests/test_options_host.py pins the table's rows to the chain it replaced).
No GPU: the sources, the public header and the binding are read and held together -- the name is set, read back and documented,
it is not also a row of the table (whose names stay those of tests/test_options_host.py), the launch site names both kernels and every instantiation of the
new one, and the parity tap the GPU test uses is declared where the binding expects it."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'pose_prefetch'


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
    assert 'int pose_prefetch = 1;' in read('pyslam_amd', 'csrc', 'ps_core.hip')        # default on
    for doc in ('INTEGRATION.md', 'DESIGN.md'):
        assert '`%s`' % NAME in read(doc), doc


def test_the_option_is_not_a_row_of_the_table():
    """(47 rows: the 46 of the chain the table replaced and the test hook "cg_force_breakdown")"""
    table = read('pyslam_amd', 'csrc', 'ps_options.h')
    assert '"%s"' % NAME not in table
    rows = re.findall(r'^\s*\{"(\w+)", ', table, re.M)
    from test_options_host import CHAIN
    assert len(rows) == 47 and set(rows) == set(CHAIN) and NAME not in CHAIN


def test_the_launch_site_chooses_by_the_option_the_chunk_and_lambda():
    host = read('pyslam_amd', 'csrc', 'ps_host_cg.h')
    assert 'if (h->pose_prefetch && h->pose_chunk <= PS_POSE_PF_OBS)' in host
    uses = re.findall(r'PS_PPF_LAUNCH\((true|false), (true|false)\);', host)
    assert sorted(uses) == [('false', 'false'), ('false', 'true'), ('true', 'false'), ('true', 'true')]
    assert len(re.findall(r'hipLaunchKernelGGL\(k_pose_pass<(?:true|false)>', host)) == 2          # option 0: the kernel before
    kernels = read('pyslam_amd', 'csrc', 'ps_k_linearize.h')
    assert '#define PS_POSE_PF_OBS 512' in kernels and 'void k_pose_pass_pf(' in kernels
    assert 'h->pose_chunk = pchunk;' in read('pyslam_amd', 'csrc', 'ps_abi_problem.h')


def test_the_parity_tap_is_declared_and_bound():
    from pyslam_amd import _native
    header = read('include', 'pyslam_hip.h')
    decl = re.search(r'int ps_debug_pose_items\((.*?)\);', header, re.S).group(1)
    assert len(decl.split(',')) == len(_native.SIGNATURES['ps_debug_pose_items'][1]) == 5
    assert 'int ps_debug_pose_items(' in read('pyslam_amd', 'csrc', 'ps_abi_solver.h')
