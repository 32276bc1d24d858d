"""The C ABI, checked once for every header (no GPU): the table imm_amd/_lib.py:ABI against include/*.h by name and by TYPE, the
ctypes mirrors of the four structs against their typedefs, the loaded library against the table, and proof that the type check can fail."""
import ctypes as C
import os
import re

import pytest

from imm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = list(L.ABI)
SCALARS = {'int': C.c_int, 'int32_t': C.c_int, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'float': C.c_float, 'double': C.c_double}
MIRRORS = {'imm_conv_desc': L.ConvDesc, 'imm_wgrad_job': L.WgradJob, 'imm_keypoint_desc': L.KeypointDesc, 'imm_opt_hparams': L.OptHParams}
# what a TYPED pointer may point to: POINTER(T) is accepted in place of c_void_p only where T is the pointee's own type
POINTEES = dict(SCALARS, uint32_t=C.c_uint32, **MIRRORS)
PROTOTYPE = re.compile(r'^(int|int64_t|const char\s*\*)\s*(imm_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;', flags=re.M)


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def strip_comments(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def declared_names(text):
    """The entry points a header declares (the start of a prototype is enough: what PROTOTYPE cannot read is then a mismatch)."""
    return sorted(set(re.findall(r'^(?:int|int64_t|const char\s*\*)\s*(imm_[a-z0-9_]+)\s*\(', strip_comments(text), flags=re.M)))


def c_type(decl):
    """'const void* const* wts' -> ('void**', 'wts'): const dropped, the stars gathered behind the base type."""
    words = re.findall(r'\w+', re.sub(r'\bconst\b', '', decl))
    return ' '.join(words[:-1]) + '*' * decl.count('*'), words[-1] if words else ''


def accepted(ctype, field=False):
    """The ctypes types that may bind the C type; none = a type outside the table, which is a mismatch."""
    if ctype.endswith('*'):
        to = ctype[:-1]
        typed = C.c_void_p if to.endswith('*') else POINTEES.get(to)
        return [C.c_void_p] + ([C.POINTER(typed)] if typed else [])
    if field and ctype in MIRRORS:
        return [MIRRORS[ctype]]                      # a struct nested by value
    return [SCALARS[ctype]] if ctype in SCALARS else []


def mismatches(text, block):
    """Every disagreement between a header's prototypes and its block of the table, as readable lines."""
    protos = {name: (ret, params) for ret, name, params in PROTOTYPE.findall(strip_comments(text))}
    out = []
    for name in sorted(set(protos) | set(block) | set(declared_names(text))):
        if name not in protos or name not in block:
            out.append('%s: %s' % (name, 'not in the table' if name in protos else 'no prototype the checker can read'))
            continue
        (ret, params), (restype, argtypes) = protos[name], block[name]
        if restype is not (C.c_char_p if 'char' in ret else SCALARS[ret]):
            out.append('%s: returns %s, bound as %s' % (name, ret, restype.__name__))
        params = [] if params.strip() in ('', 'void') else params.split(',')
        if len(params) != len(argtypes):
            out.append('%s: %d parameters, %d bound' % (name, len(params), len(argtypes)))
            continue
        for i, (param, bound) in enumerate(zip(params, argtypes)):
            if bound not in accepted(c_type(param)[0]):
                out.append('%s: parameter %d `%s` bound as %s' % (name, i, ' '.join(param.split()), bound.__name__))
    return out


def struct_fields(text, cname):
    """[(field, C type)] of `typedef struct cname {...} cname;` in declaration order."""
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), strip_comments(text), flags=re.S).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        first, *more = decl.split(',')
        ctype, name = c_type(first)
        out += [(name, ctype)] + [(m.strip(), ctype if re.fullmatch(r'\s*\w+\s*', m) else '?') for m in more]
    return out


def struct_mismatches(text, cname, fields):
    """Every disagreement between a typedef of the header and the _fields_ of its ctypes mirror."""
    want = struct_fields(text, cname)
    if [n for n, _ in want] != [n for n, _ in fields]:
        return ['%s: fields %s, mirrored as %s' % (cname, [n for n, _ in want], [n for n, _ in fields])]
    return ['%s.%s: `%s` mirrored as %s' % (cname, n, ctype, bound.__name__)
            for (n, ctype), (_, bound) in zip(want, fields) if bound not in accepted(ctype, field=True)]


@pytest.fixture(scope='module')
def lib():
    return L.load()


def test_the_table_lists_the_headers_in_the_order_imm_hip_h_includes_them():
    main = read('include', 'imm_hip.h')
    assert HEADERS == ['imm_hip.h'] + re.findall(r'^#include "(imm_[a-z0-9_]+\.h)"', main, flags=re.M)
    assert sorted(HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, 'include')) if f.endswith('.h'))


@pytest.mark.parametrize('header', HEADERS)
def test_header_table_and_library_agree(header, lib):
    text, block = read('include', header), L.ABI[header]
    assert declared_names(text) == L.symbols(header), set(declared_names(text)) ^ set(block)
    for name, (restype, argtypes) in block.items():
        fn = getattr(lib, name)                                           # resolves
        assert L.signature(name) == (restype, argtypes)
        assert fn.restype is restype and list(fn.argtypes or ()) == argtypes, name
    assert mismatches(text, block) == []                                  # by type, not by count
    if header != 'imm_hip.h':
        # a feature header's entry points are named in a comment block of imm_hip.h and nowhere else in it, never before a
        # parenthesis: imm_hip.h's own count of entry points stays
        main = read('include', 'imm_hip.h')
        bare = re.sub(r'#include "[^"]*"', '', re.sub(r'/\*.*?\*/', '', main, flags=re.S))
        comments = '\n'.join(re.findall(r'/\*.*?\*/', main, flags=re.S))
        for name in block:
            assert name not in bare, '%s is declared in imm_hip.h itself' % name
            assert name in comments, '%s is not named in a comment block of imm_hip.h' % name
            assert not re.search(r'%s\s*\(' % name, main), '%s is followed by a parenthesis in imm_hip.h' % name


def test_no_entry_point_is_declared_by_two_headers():
    names = [n for block in L.ABI.values() for n in block]
    assert len(names) == len(set(names)) == len(L.symbols()), sorted(n for n in set(names) if names.count(n) > 1)
    for i, a in enumerate(HEADERS):
        for b in HEADERS[i + 1:]:
            assert not set(L.ABI[a]) & set(L.ABI[b]), (a, b)
            assert not set(declared_names(read('include', a))) & set(declared_names(read('include', b))), (a, b)


def test_abi_version_and_the_count_of_imm_hip_h(lib):
    main = read('include', 'imm_hip.h')
    assert int(re.search(r'#define IMM_ABI_VERSION (\d+)', main).group(1)) == L.ABI_VERSION == lib.imm_abi_version()
    assert len(set(re.findall(r'\b(imm_[a-z0-9_]+)\s*\(', main))) == 93 == len(L.symbols('imm_hip.h'))
    assert '93 entry points' in read('INTEGRATION.md')


def test_struct_mirrors_have_the_headers_fields_in_the_headers_order():
    main = read('include', 'imm_hip.h')
    assert sorted(re.findall(r'typedef struct (imm_\w+)', strip_comments(main))) == sorted(MIRRORS)
    assert not any('typedef struct' in strip_comments(read('include', h)) for h in HEADERS[1:]), 'a struct without a checked mirror'
    for cname, mirror in MIRRORS.items():
        assert struct_mismatches(main, cname, mirror._fields_) == []


def test_build_resolves_every_symbol_of_the_table():
    assert 'for name in _lib.symbols():' in read('__graft_entry__.py')


def test_the_checker_reports_planted_errors():
    """Without this the type check could pass vacuously: five errors planted in copies of the real table, each one reported."""
    def planted(header, name, edit):
        block = {n: (r, list(a)) for n, (r, a) in L.ABI[header].items()}
        block[name] = edit(*block[name])
        text = read('include', header)
        assert mismatches(text, L.ABI[header]) == []
        found = mismatches(text, block)
        assert len(found) == 1 and found[0].startswith(name + ':'), found
        return found[0]

    def swap(args, old, new):
        i = args.index(old)
        return args[:i] + [new] + args[i + 1:]

    assert 'bound as c_float' in planted('imm_track.h', 'imm_track_step', lambda r, a: (r, swap(a, C.c_double, C.c_float)))
    assert '28 parameters, 27 bound' in planted('imm_seam.h', 'imm_seam_fit', lambda r, a: (r, a[:-1]))
    assert 'parameter 0' in planted('imm_clip.h', 'imm_clip_rows', lambda r, a: (r, swap(a, C.c_void_p, C.c_int)))
    assert 'returns int64_t' in planted('imm_hip.h', 'imm_conv2d_workspace_bytes', lambda r, a: (C.c_int, a))
    main, fields = read('include', 'imm_hip.h'), list(L.OptHParams._fields_)
    assert [n for n, _ in fields[2:4]] == ['lr_step', 'lr_multiple']
    fields[2], fields[3] = fields[3], fields[2]
    found = struct_mismatches(main, 'imm_opt_hparams', fields)
    assert len(found) == 1 and found[0].startswith('imm_opt_hparams: fields'), found
    # the same two exchanged in name only: the types then sit where the header has the other's
    renamed = list(L.OptHParams._fields_)
    renamed[2], renamed[3] = ('lr_step', C.c_float), ('lr_multiple', C.c_int32)
    assert len(struct_mismatches(main, 'imm_opt_hparams', renamed)) == 2
