"""The host-side argument handling of the pair-potential entries (sella_amd/csrc/pair_pot.h) as a stand-alone program
(tests/pair_args_check.cpp, its own main) built with the host sanitizers: statically linked, nothing is loaded into
Python and no GPU is touched."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def host_compiler():
    for cxx in (os.environ.get('HOSTEMU_CXX'), '/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++')):
        if cxx and os.path.exists(cxx):
            return cxx
    return None


def test_pair_argument_handling_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip('no clang++ to build the stand-alone program with')
    exe = str(tmp_path / 'pair_args_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', os.path.join(REPO, 'tests', 'pair_args_check.cpp'), '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = run.stdout.decode(errors='replace')
    assert run.returncode == 0 and 'pair_args_check ok' in out, out
