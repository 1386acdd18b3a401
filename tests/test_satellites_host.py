"""The binding of the feature libraries beside libdurf_hip.so, one test for all of them: for every name in _lib.SATELLITES,
include/durf_<name>.h, durf_amd/_<name>_sigs.py and libdurf_<name>.so's dynamic symbol table name the same entry points, which
no other library of the project -- older or newer -- names; the generated files are current; and the Makefile, the loader, the
headers and the tables list the same libraries.  What each library's entry points are stays with its own
tests/test_<name>_host.py."""
import glob
import os
import re
import subprocess
import sys

import pytest

from durf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name):
    hdr = open(os.path.join(ROOT, 'include', 'durf_%s.h' % name)).read()
    body = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    return set(re.findall(r'\b(durf_[a-z0-9_]+)\s*\(', body))


def _dynamic(path, only_entries):
    out = subprocess.run(['nm', '-D', '--defined-only', path], check=True, capture_output=True, text=True).stdout
    if only_entries:
        return {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln and ln.split()[-1].startswith('durf_')}
    return {ln.split()[-1] for ln in out.splitlines()}


@pytest.mark.parametrize('name', _lib.SATELLITES)
def test_header_table_and_symbol_table_agree_and_are_this_librarys_alone(name):
    declared = _declared(name)
    assert declared and declared == set(_lib.satellite_symbols(name))
    L = _lib.satellite(name)
    assert all(hasattr(L, s) for s in declared)
    assert _dynamic(_lib.satellite_path(name), True) == declared
    for other in _lib.SATELLITES:
        if other != name:
            assert not declared & set(_lib.satellite_symbols(other)), other
            assert not declared & _dynamic(_lib.satellite_path(other), False), other
    assert not declared & set(_lib.symbols())
    assert not declared & _dynamic(_lib.LIB_PATH, False), 'libdurf_hip.so keeps its own set of entry points'
    # the scan kernel of csrc/scan.h is compiled into several libraries of one process: each launches its own copy
    assert not [s for s in _dynamic(_lib.satellite_path(name), False) if 'k_scan' in s]


def test_the_generated_files_are_current():
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_integration_stub.py'), '--check'], cwd=ROOT).returncode == 0


def test_makefile_loader_headers_and_tables_list_the_same_libraries():
    mk = open(os.path.join(ROOT, 'durf_amd', 'csrc', 'Makefile')).read()
    in_makefile = re.search(r'^SATELLITES\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert tuple(in_makefile) == _lib.SATELLITES and len(set(in_makefile)) == len(in_makefile)
    headers = {os.path.basename(p)[len('durf_'):-len('.h')] for p in glob.glob(os.path.join(ROOT, 'include', 'durf_*.h'))} - {'hip'}
    tables = {os.path.basename(p)[1:-len('_sigs.py')] for p in glob.glob(os.path.join(ROOT, 'durf_amd', '_*_sigs.py'))}
    assert headers == tables == set(_lib.SATELLITES)
    with pytest.raises(KeyError):
        _lib.satellite('hip')
    assert _lib.lidar_lib() is _lib.satellite('lidar') and _lib.LIDAR_LIB_PATH == _lib.satellite_path('lidar')
    assert _lib.geom_symbols() == _lib.satellite_symbols('geom')
    with pytest.raises(AttributeError):
        _lib.nothing_lib
