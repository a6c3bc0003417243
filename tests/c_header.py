"""What the C compiler makes of include/simplyp.h: the values of constant expressions (sizeof, offsetof, enums, macros)."""

import os
import subprocess
import tempfile

from simplyp_amd import engine

HEADER = os.path.join(engine.INCLUDE, 'simplyp.h')


def header_text():
    with open(HEADER) as fh:
        return fh.read()


def c_values(exprs):
    """{expression: its value as an int} for C constant expressions over simplyp.h, all from one compiled program."""
    exprs = list(exprs)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void) {']
    lines += ['    printf("%%lld %s\\n", (long long)(%s));' % (e, e) for e in exprs]
    lines += ['    return 0;', '}', '']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'values.c'), os.path.join(tmp, 'values')
        with open(src, 'w') as fh:
            fh.write('\n'.join(lines))
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-o', exe, src])
        out = subprocess.check_output([exe], text=True)
    got = {name: int(value) for value, name in (l.split(' ', 1) for l in out.splitlines())}
    assert list(got) == exprs
    return got
