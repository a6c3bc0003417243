"""The stand-alone host programs of tests/*_host_main.cpp: each includes headers of simplyp_amd/csrc, is built with the host
compiler under AddressSanitizer and UBSan, and runs as a child process; the sanitizers abort the child on any finding."""

import atexit
import functools
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ME = 'entry_under_test'                 # the entry name the programs hand to the argument checks


@functools.lru_cache(maxsize=None)
def build(source_name, *more_flags):
    """The path of the program built from tests/<source_name>; built once per process."""
    work = tempfile.mkdtemp(prefix='simplyp_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    exe = os.path.join(work, os.path.splitext(source_name)[0])
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all'] + list(more_flags) + ['-o', exe, os.path.join(HERE, source_name)])
    return exe


def case_runner(exe, timeout):
    def run(cases):
        """cases: lines of text -> per case (rc, rest of its line)."""
        p = subprocess.run([exe], input='\n'.join(cases) + '\n', capture_output=True, text=True, timeout=timeout)
        assert p.returncode == 0 and p.stderr == '', p.stderr
        lines = p.stdout.splitlines()
        assert len(lines) == len(cases)
        return [(int(l.split(' ', 1)[0]), l.split(' ', 1)[1] if ' ' in l else '') for l in lines]
    return run


def rejected(results):
    for rc, msg in results:
        assert rc == -1 and msg.startswith(ME + ': '), (rc, msg)
