"""The host descriptor structs and capacity constants that _lib.parse_structs binds from include/srec.h and
include/srec_hg.h: their layout is the host C compiler's, nothing of the headers is left out, and what the parser
cannot lay out it refuses.  CPU only: the generated program is plain host C."""
import ctypes
import os
import re
import subprocess

import pytest

from util import ROOT, pkg

INCLUDE = os.path.join(ROOT, 'include')


def _stripped_headers():
    src = '\n'.join(open(os.path.join(INCLUDE, h)).read() for h in ('srec.h', 'srec_hg.h'))
    return re.sub(r'/\*.*?\*/|//[^\n]*', '', src, flags=re.S)


def test_struct_layout_equals_the_compilers(tmp_path):
    """sizeof of every struct and offsetof of every member, as g++ lays the headers out, equal ctypes.sizeof and the field
    offsets of the parsed classes: 241 members + 11 structs = 252 values.  Offsets alone cannot see two mistakes, so each
    member's size is compared as well (a `long` between two pointers keeps every offset whatever width the parser gives it:
    srec_step_prep_desc.box_cap), and of every array member the size of element [0] (A[P][S] and A[S][P] are equally large)."""
    L = pkg('_lib')
    lines, want_layout, want_size, want_row = [], {}, {}, {}
    for name, cls in L.STRUCTS.items():
        lines.append('printf("L %s %%zu\\n", sizeof(%s));' % (name, name))
        want_layout[name] = ctypes.sizeof(cls)
        for f, ty in cls._fields_:
            lines.append('printf("L %s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
            lines.append('printf("S %s.%s %%zu\\n", sizeof(((%s*)0)->%s));' % (name, f, name, f))
            want_layout['%s.%s' % (name, f)] = getattr(cls, f).offset
            want_size['%s.%s' % (name, f)] = getattr(cls, f).size
            if issubclass(ty, ctypes.Array):
                lines.append('printf("R %s.%s %%zu\\n", sizeof(((%s*)0)->%s[0]));' % (name, f, name, f))
                want_row['%s.%s' % (name, f)] = ctypes.sizeof(ty._type_)
    src = tmp_path / 'layout.cpp'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srec.h"\nint main() {\n%s\nreturn 0;\n}\n' % '\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.run(['g++', '-I', INCLUDE, str(src), '-o', exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split('\n')
    got_layout = {k: int(v) for t, k, v in (ln.split() for ln in out if ln) if t == 'L'}
    got_size = {k: int(v) for t, k, v in (ln.split() for ln in out if ln) if t == 'S'}
    assert got_layout == want_layout, sorted(k for k in want_layout if got_layout.get(k) != want_layout[k])
    assert len(got_layout) == 273 and len(L.STRUCTS) == 12 and got_layout['srec_served'] == 136
    assert got_size == want_size, sorted(k for k in want_size if got_size.get(k) != want_size[k])
    assert len(got_size) == 261
    got_row = {k: int(v) for t, k, v in (ln.split() for ln in out if ln) if t == 'R'}
    assert got_row == want_row and len(got_row) > 100, sorted(k for k in want_row if got_row.get(k) != want_row[k])


def test_every_struct_and_constant_of_the_headers_is_bound():
    L = pkg('_lib')
    src = _stripped_headers()
    assert len(L.STRUCTS) == len(re.findall(r'\btypedef\s+struct\b', src)) == 12
    defines = re.findall(r'#\s*define\s+(SREC_\w+)[ \t]+(\S+)', src)
    ints = {n: int(v, 0) for n, v in defines if re.fullmatch(r'-?(0[xX][0-9a-fA-F]+|\d+)', v)}
    assert len(ints) >= 16 and ints == L.CONST
    assert L.CONST['SREC_HG_MAXT'] == 4 and L.CONST['SREC_G16_MAXP'] == 16 and L.CONST['SREC_BAD_ARG'] == 1001


def test_parser_lays_out_what_the_headers_use():
    L = pkg('_lib')
    const, st = L.parse_structs('#define SREC_P 3\n#define SREC_S 2\n/* int gone; */\n'
                                'typedef struct tag { const float* A[SREC_P][SREC_S]; int a[SREC_P], b, c[2]; // x\n'
                                ' float* const* p; long n; float f; } srec_t;')
    assert const == {'SREC_P': 3, 'SREC_S': 2}
    t = st['srec_t']
    assert [f for f, _ in t._fields_] == ['A', 'a', 'b', 'c', 'p', 'n', 'f']
    assert len(t().A) == 3 and len(t().A[0]) == 2 and t.A.size == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert (t.a.size, t.b.size, t.c.size, t.p.size, t.n.size, t.f.size) == (12, 4, 8, ctypes.sizeof(ctypes.c_void_p),
                                                                           ctypes.sizeof(ctypes.c_long), 4)


@pytest.mark.parametrize('member', ['double x;',                       # unknown base type
                                    'unsigned int x;',
                                    'int x[SREC_NOPE];',               # undefined extent name
                                    'int x : 3;',                      # bit-field
                                    'struct { int a; } x;',            # nested struct
                                    'union { int a; float b; } x;',
                                    'int (*x)(int);',                  # function pointer
                                    'int x[2][2][2];',                 # more dimensions than the rules cover
                                    'int* x, y;',                      # y is no pointer in C
                                    'int x[0];'])
def test_parser_refuses_what_it_cannot_lay_out(member):
    L = pkg('_lib')
    with pytest.raises(ValueError):
        L.parse_structs('#define SREC_N 4\ntypedef struct { int ok[SREC_N]; %s float tail; } srec_t;' % member)


def test_parser_refuses_a_typedef_it_does_not_recognise():
    L = pkg('_lib')
    with pytest.raises(ValueError):
        L.parse_structs('struct srec_s { int a; };\ntypedef struct srec_s srec_t;')
