"""ctypes binding of libsrec_hip.so.

The prototypes are parsed from include/srec.h, so every symbol the header declares
is bound (and a missing export fails at import) and takes exactly the declared number of
arguments (TypeError ahead of the call otherwise).  The host descriptor structs and the
SREC_* capacity constants are bound from include/srec.h and include/srec_hg.h in the same
way (STRUCTS, CONST): to extend a struct, edit the header only.  There is NO fallback: if
the HIP library is absent, or a tensor is not on the GPU, the product path raises.
"""
import ctypes
import os
import re

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'srec.h')
HEADERS = (HEADER, os.path.join(os.path.dirname(HERE), 'include', 'srec_hg.h'))
LIB_PATH = os.path.join(HERE, 'libsrec_hip.so')

_CT = {
    'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float,
    'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'const int*': ctypes.c_void_p,
    'int*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'const float* const*': ctypes.c_void_p,
    'unsigned long long': ctypes.c_ulonglong, 'unsigned*': ctypes.c_void_p,
    'unsigned char*': ctypes.c_void_p, 'const unsigned char*': ctypes.c_void_p, 'const long long*': ctypes.c_void_p, 'long long*': ctypes.c_void_p, 'const void*': ctypes.c_void_p, 'long*': ctypes.c_void_p, 'const long*': ctypes.c_void_p,
}


def parse_header(path=HEADER):
    """-> {name: [(ctype_string, argname), ...]} for every `int srec_*(...)` declaration."""
    src = open(path).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for m in re.finditer(r'\bint\s+(srec_\w+)\s*\(([^)]*)\)\s*;', src):
        args = []
        for a in m.group(2).split(','):
            a = ' '.join(a.split())
            mm = re.match(r'^(.*?)(\w+)$', a)
            ty = mm.group(1).strip().replace(' *', '*')
            args.append((ty, mm.group(2)))
        protos[m.group(1)] = args
    return protos


_BASE = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float}


def parse_structs(src=None):
    """header text (default: include/srec.h + include/srec_hg.h) -> ({SREC_* define: int}, {struct name: ctypes structure
    class}) for every `#define SREC_* <integer>` and every `typedef struct [tag] { ... } name;`.  Members: int / long /
    float, anything with a `*` (c_void_p), one or two array extents (literal or define; the first is the outermost), several
    declarators per declaration.  Anything else raises: a layout guessed wrong sends device pointers to the wrong offsets."""
    if src is None:
        src = '\n'.join(open(p).read() for p in HEADERS)
    src = re.sub(r'/\*.*?\*/|//[^\n]*', '', src, flags=re.S)
    const = {m.group(1): int(m.group(2), 0)
             for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(SREC_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$', src, re.M)}
    structs = {}
    for m in re.finditer(r'\btypedef\s+struct\b\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', src, re.S):
        body, name, fields = m.group(1), m.group(2), []
        for decl in filter(None, (' '.join(d.split()) for d in body.split(';'))):
            first, *more = [d.strip() for d in decl.split(',')]
            mm = re.match(r'^([\w\s*]+?)\s*\b(\w+)((?:\s*\[\s*\w+\s*\]){0,2})$', first)
            if re.search(r'[{}:()]', decl) or mm is None:
                raise ValueError('%s: cannot lay out `%s` (nested struct / union, bit-field, function pointer?)' % (name, decl))
            base = ' '.join(t for t in mm.group(1).replace('*', ' * ').split() if t != 'const')
            if '*' in base and more:
                raise ValueError('%s: `%s` declares several members of a pointer type' % (name, decl))
            if '*' not in base and base not in _BASE:
                raise ValueError('%s: unknown member type `%s` in `%s`' % (name, base, decl))
            for d in [mm.group(2) + mm.group(3)] + more:
                dm = re.match(r'^(\w+)((?:\s*\[\s*\w+\s*\]){0,2})$', d)
                if dm is None:
                    raise ValueError('%s: cannot lay out `%s` in `%s`' % (name, d, decl))
                ct = ctypes.c_void_p if '*' in base else _BASE[base]
                for e in reversed(re.findall(r'\w+', dm.group(2))):
                    if not (e.isdigit() or e in const) or int(const.get(e, e)) <= 0:
                        raise ValueError('%s: array extent `%s` of `%s` is no positive literal or SREC_* define' % (name, e, d))
                    ct = ct * int(const.get(e, e))
                fields.append((dm.group(1), ct))
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields, '__doc__': 'host struct %s of the C headers' % name})
    if len(structs) != len(re.findall(r'\btypedef\s+struct\b', src)):
        raise ValueError('a `typedef struct` of the headers was not understood (parsed: %s)' % sorted(structs))
    return const, structs


CONST, STRUCTS = parse_structs()
# the descriptor of the multi-table served score has a header of its own (include/srec_ens.h, included by srec.h): bound from
# there in the same way, beside CONST / STRUCTS, not among them
ENS_HEADER = os.path.join(os.path.dirname(HERE), 'include', 'srec_ens.h')
ENS_CONST, ENS_STRUCTS = parse_structs(open(ENS_HEADER).read())


class _Lib:
    def __init__(self):
        self._dll = None
        self.protos = parse_header()

    def load(self):
        if self._dll is not None:
            return self._dll
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'libsrec_hip.so is missing (%s): build it with `python -c "import __graft_entry__ as g; g.build()"`. '
                'There is no CPU fallback for the product path.' % LIB_PATH)
        dll = ctypes.CDLL(LIB_PATH)
        for name, args in self.protos.items():
            getattr(dll, name)                 # AttributeError if the export is missing
            # bound WITH parameter flags: ctypes then takes exactly the declared number of arguments (TypeError otherwise,
            # ahead of the call).  A plain cdecl binding lets surplus arguments through, and a caller written against an
            # older positional prototype would hand its first pointer to a `const void* desc` / `served`, which is followed
            types = [_CT[t] for t, _ in args]
            fn = ctypes.CFUNCTYPE(ctypes.c_int, *types)((name, dll), tuple((1, n) for _, n in args))
            fn.argtypes = types
            setattr(dll, name, fn)
        self._dll = dll
        return dll

    def __getattr__(self, name):
        if name.startswith('srec_'):
            fn = getattr(self.load(), name)

            def call(*a):
                rc = fn(*a)
                if rc != 0:
                    raise RuntimeError('%s failed with status %d%s' % (
                        name, rc, ' (bad argument: alignment / dimension contract of include/srec.h)' if rc == 1001 else
                        ' (hipError_t)'))
            return call
        raise AttributeError(name)


lib = _Lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """device pointer of a tensor (None -> NULL).  Raises for CPU tensors: no fallback."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('sessionrec-pytorch_amd ops need GPU (HIP) tensors; got a %s tensor' % t.device)
    return t.data_ptr()


def ptr_array(ts):
    """HOST array of the device pointers of `ts` (None -> NULL); the caller keeps it alive across the lib.srec_* call"""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def f32c(t):
    assert t.dtype == torch.float32, t.dtype
    return t if t.is_contiguous() else t.contiguous()
