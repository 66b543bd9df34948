"""The host descriptor of the served score (include/srec.h: srec_served) for the CPU ABI tests: its members in order, and a
call helper that fills one from the `good` / `change` dicts those tests keep - fake pointers that are never followed, since
every refusal happens ahead of the launch."""
import ctypes

from util import pkg

P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
MEMBERS = [('sr', P), ('ld_sr', I), ('comp_stride', L), ('E', P), ('ld_e', I), ('cs', P), ('off_ex', P), ('off_in', P),
           ('listed', P), ('L', I), ('listed_mode', I), ('id_lo', L), ('B', I), ('V', I), ('d', I), ('C', I),
           ('bias', P), ('ld_bias', L), ('group', P), ('G', I)]
NO_BIAS = dict(bias=None, ld_bias=0, group=None, G=1)          # what a call without a bias carries


def served(args):
    """srec_served from the entries of `args` that name its members (a call without a bias: NO_BIAS)"""
    args = {**NO_BIAS, **args}
    return pkg('_lib').STRUCTS['srec_served'](*[args[n] for n, _ in MEMBERS])


def call(fn, rest, args, null=False):
    """fn(&served(args), *[args[n] for n in rest]); null: a NULL descriptor instead"""
    desc = served(args)
    return fn(None if null else ctypes.addressof(desc), *[args[n] for n in rest])


def proto(name):
    """[(C type, argument name)] of an entry point as the header declares it"""
    return pkg('_lib').parse_header()[name]
